import re, sys
# usage: isa_pattern.py DISASSEMBLY KERNEL_SYMBOL_SUBSTRING
# Compact op pattern of one kernel out of `llvm-objdump -d --mcpu=gfx950` of the unbundled gfx950 object
# (hipcc <_build.hip_flags()> --cuda-device-only --no-gpu-bundle-output -c FILE.hip):
# M mfma, R ds_read, W ds_write, GL/GS global or buffer load/store, DMA buffer load to LDS,
# Vn a run of n VALU, [..] s_waitcnt, ==BAR== s_barrier, <..> branch
path, key = sys.argv[1], sys.argv[2]
cur = None; out = []; valu = 0
def flush():
    global valu
    if valu: out.append(f"V{valu}"); valu = 0
for line in open(path):
    m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
    if m: cur = m.group(1); continue
    if cur is None or key not in cur: continue
    t = line.strip().split("//")[0].split()
    if not t: continue
    op = t[0]
    if op.startswith("v_mfma"): flush(); out.append("M")
    elif op.startswith("ds_read"): flush(); out.append("R")
    elif op.startswith("ds_write"): flush(); out.append("W")
    elif op == "s_waitcnt": flush(); out.append("[" + "".join(t[1:]) + "]")
    elif op == "s_barrier": flush(); out.append("\n==BAR==\n")
    elif op.startswith("global_load") or op.startswith("buffer_load"): flush(); out.append("GL" if "lds" not in line else "DMA")
    elif op.startswith("global_store") or op.startswith("buffer_store"): flush(); out.append("GS")
    elif op.startswith("s_cbranch") or op.startswith("s_branch"): flush(); out.append("<" + op[2:] + ">")
    elif op.startswith("v_"): valu += 1
flush()
print(" ".join(out))
