"""Audio models: the ``AudioSpectrogram`` / ``Mfcc`` / ``DecodeWav`` ops, the front-end kernel of
``kernels/audio.hip``, its launchers, the lowering and the zoo keyword spotter.

**The mirror.**  The reference is a float64 mirror written with plain loops from the ops'
definitions (``_mirror``): frames ``[f stride, f stride + window)`` times the periodic Hann
window, zero-padded to ``N``, ``|rfft|^2``; the mel bank bin by bin in ascending order on
``sqrt`` of the power; ``log(max(., 1e-12))``; the DCT-II with ``sqrt(2 / C)``.

**Data**, seeded from the case: noise of amplitude 0.3 plus a chirp from 100 Hz to 45 % of the
sample rate, per clip.  The input is broadband so that no mel channel holds only leakage: for a
pure tone some channels lie 1e-6 below the peak and the log magnifies their fp32 error to ~3e-3,
so the tone case is checked at the spectrogram, not at the coefficients.

**The tolerance** is measured, not chosen (``_host_error``): ``E_m`` is the largest absolute
MFCC difference between the launcher's fp32 host path (``torch.fft.rfft``, the same tables) and
the mirror over the GPU cases, ``E_s`` the largest spectrogram difference (both forms, the tone
case included) relative to each frame's peak.  The GPU tests allow ``8 E_m`` and ``8 E_s``: the
kernel's radix-2 FFT and FMA contraction differ from pocketfft's, the precision class is the
same.  Measured on the CPU:

    E_m = 7.6e-06 .. 9.8e-06 (it depends on the host's FFT; coefficients span up to +-47),
    E_s = 3.2e-07 .. 3.5e-07; GPU bounds 6.1e-05 .. 7.8e-05 and 2.6e-06 .. 2.8e-06

On the MI355X the kernel differs from the mirror by at most 9.8e-06 in a coefficient and 2.9e-07 of the
peak in a spectrogram: the host path's class, an eighth of the bounds.

``test_tolerance_cannot_hide_an_indexing_bug`` asserts that mirrors with one deliberate fault
each differ from the true mirror by more than ten times the GPU bound.
"""
import functools
import io
import math
import wave
import zlib

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph import ops_nn
from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K
from flink_tensorflow_amd.types.tensor import StringTensor

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100          # output sentinel: exact in bf16 and fp32, far above any result
NAN = float("nan")
FPW = K.AUDIO_FRAMES_PER_WG

# (S, B, window, stride, C, D, rate, lo, hi)
CASES = (
    (200, 1, 200, 80, 20, 13, 8000, 20, 3800),        # one frame, alone in its pair
    (700, 3, 200, 77, 20, 13, 8000, 20, 3800),        # 7 frames, unaligned stride
    (1029, 2, 256, 256, 20, 20, 8000, 20, 3800),      # no zero padding, no overlap, ignored tail
    (1500, 2, 200, 300, 20, 13, 8000, 20, 3800),      # stride above the window
    (2080, 5, 480, 160, 40, 40, 16000, 20, 4000),     # the workload's configuration, 11 frames
    (3200, 2, 640, 320, 40, 13, 16000, 20, 7600),     # N = 1024
    (4851, 1, 1323, 441, 64, 20, 44100, 20, 16000),   # N = 2048
    (200 + FPW * 80, 2, 200, 80, 20, 13, 8000, 20, 3800),            # one frame above a workgroup's count
    (200 + (2 * FPW - 2) * 80, 2, 200, 80, 20, 13, 8000, 20, 3800),  # one below twice that count
)
WORKLOAD = CASES[4]
SUBSET = (CASES[1], CASES[4], CASES[6], CASES[7])     # odd frame count, the workload, N = 2048, two workgroups


def _case_id(c):
    S, B, w, st, C, D, rate, lo, hi = c
    return f"S{S}xB{B}-w{w}s{st}-C{C}D{D}-{rate}Hz"


def _frames(c):
    return K.audio_frames(c[0], c[2], c[3])


# ----------------------------------------------------------------------------------- the mirror
def _bank(bins, rate, lo, hi, C, shift=0):
    """(start, end, band [bins], weight [bins]) from the definition, float64, plain loops."""
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)  # noqa: E731
    mlo, mhi = mel(lo), mel(hi)
    centre = [mlo + (mhi - mlo) / (C + 1) * (i + 1) for i in range(C + 1)]
    hz = 0.5 * rate / (bins - 1)
    start, end = int(1.5 + lo / hz), int(hi / hz)
    band, weight = [-2] * bins, [0.0] * bins
    for i in range(start, end + 1):
        m = mel(i * hz)
        c = -1
        while c + 1 < C and centre[c + 1] < m:
            c += 1
        band[i] = c + shift
        weight[i] = (centre[c + 1] - m) / (centre[c + 1] - (centre[c] if c >= 0 else mlo))
    return start, end, band, weight


def _mirror_spec(x, window, stride, fault=None):
    """float64 power spectrogram ``[B, F, N/2 + 1]`` of ``x [S, B]``."""
    x = np.asarray(x, dtype=np.float64)
    S, B = x.shape
    N = 1
    while N < window:
        N *= 2
    F_ = 1 + (S - window) // stride if S >= window else 0
    out = np.zeros((B, F_, N // 2 + 1))
    n = np.arange(window)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / window)
    for b in range(B):
        for f in range(F_):
            ff = f ^ 1 if fault == "pair_swap" and (f ^ 1) < F_ else f
            s0 = ff * stride + (1 if fault == "frame_offset" else 0)
            buf = np.zeros(N)
            if fault == "window_stretch":  # N samples under a Hann window of N points
                seg = x[s0:s0 + N, b]
                buf[:len(seg)] = seg * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N))[:len(seg)]
            else:
                seg = x[s0:s0 + window, b]
                buf[:len(seg)] = seg * hann[:len(seg)]
            z = np.fft.rfft(buf)
            out[b, f] = z.real ** 2 + z.imag ** 2
    return out


def _mirror_mfcc(power, rate, lo, hi, C, D, fault=None):
    """float64 ``Mfcc`` of a power spectrogram ``[B, F, bins]`` with plain loops."""
    B, F_, bins = power.shape
    start, end, band, weight = _bank(bins, rate, lo, hi, C, shift=1 if fault == "band_shift" else 0)
    out = np.zeros((B, F_, D))
    for b in range(B):
        for f in range(F_):
            mel = [0.0] * C
            for i in range(start, end + 1):
                v = power[b, f, i] if fault == "no_sqrt" else math.sqrt(power[b, f, i])
                c = band[i]
                if 0 <= c < C:
                    mel[c] += v * weight[i]
                if 0 <= c + 1 < C:
                    mel[c + 1] += v - v * weight[i]
            lm = [math.log(max(m, 1e-12)) for m in mel]
            half = 0.0 if fault == "dct_no_half" else 0.5
            for d in range(D):
                out[b, f, d] = sum(math.sqrt(2.0 / C) * math.cos(d * math.pi / C * (j + half)) * lm[j] for j in range(C))
    return out


@functools.lru_cache(maxsize=None)
def _data(case):
    """``x [S, B]`` fp32: noise of amplitude 0.3 plus a chirp; every mel channel of the case is non-empty."""
    S, B, w, st, C, D, rate, lo, hi = case
    assert K.mfcc_eligible(S, w, st, C, D, rate, lo, hi), case
    start, end, band, _ = _bank(K.audio_fft_length(w) // 2 + 1, rate, lo, hi, C)
    hit = {band[i] for i in range(start, end + 1)} | {band[i] + 1 for i in range(start, end + 1)}
    assert set(range(C)) <= hit, "a mel channel of the case receives no bin"
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    t = torch.arange(S, dtype=F64) / rate
    dur = S / rate
    x = torch.empty((S, B), dtype=F64)
    for b in range(B):
        f1 = 0.45 * rate * (b + 1) / B
        x[:, b] = 0.3 * torch.randn(S, generator=g, dtype=F64) + 0.4 * torch.sin(
            2 * math.pi * (100.0 * t + 0.5 * (f1 - 100.0) * t * t / dur))
    return x.float()


@functools.lru_cache(maxsize=None)
def _tone():
    """A pure 1 kHz tone in the workload's configuration, ``[S, 2]`` (two amplitudes)."""
    S, rate = WORKLOAD[0], WORKLOAD[6]
    t = torch.arange(S, dtype=F64) / rate
    return torch.stack([0.5 * torch.sin(2 * math.pi * 1000.0 * t), 0.05 * torch.sin(2 * math.pi * 1000.0 * t + 1.0)], 1).float()


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(power spectrogram, MFCC) of the case's data from the mirror, float64 tensors; never modified."""
    S, B, w, st, C, D, rate, lo, hi = case
    p = _mirror_spec(_data(case).numpy(), w, st)
    return torch.from_numpy(p), torch.from_numpy(_mirror_mfcc(p, rate, lo, hi, C, D))


@functools.lru_cache(maxsize=None)
def _ref_tone():
    return torch.from_numpy(_mirror_spec(_tone().numpy(), WORKLOAD[2], WORKLOAD[3]))


def _tables(case, dev=None):
    S, B, w, st, C, D, rate, lo, hi = case
    return K.mfcc_tables(w, rate, lo, hi, C, D, device=dev)


def _spec_err(got, ref_power, squared):
    """Largest difference relative to each frame's peak (power or magnitude)."""
    ref = ref_power if squared else ref_power.sqrt()
    return float(((got.to(F64) - ref).abs().amax(-1) / ref.amax(-1)).max())


@functools.lru_cache(maxsize=None)
def _host_error():
    """(E_m, E_s): the launchers' fp32 host path against the mirror over the GPU cases and the tone."""
    em = es = 0.0
    for case in CASES:
        x, tb = _data(case), _tables(case)
        p, m = _ref(case)
        em = max(em, float((K.audio_mfcc(x, tb, case[3]).to(F64) - m).abs().max()))
        for sq in (True, False):
            es = max(es, _spec_err(K.audio_spectrogram(x, tb, case[3], sq), p, sq))
    tb = _tables(WORKLOAD)
    for sq in (True, False):
        es = max(es, _spec_err(K.audio_spectrogram(_tone(), tb, WORKLOAD[3], sq), _ref_tone(), sq))
    return em, es


def _bounds():
    """The GPU bounds ``(8 E_m, 8 E_s)``."""
    em, es = _host_error()
    return 8 * em, 8 * es


# =================================================================================== CPU: the ops
@pytest.mark.parametrize("N,k0", ((256, 20), (512, 3)))
def test_spectrogram_of_a_cosine_at_an_exact_bin(N, k0):
    """``cos(2 pi k0 n / N)`` under the periodic Hann window of ``N`` points: the spectrum is
    ``N/4`` at ``k0`` and ``-N/8`` at ``k0 +- 1``, so the power is ``N^2/16``, ``N^2/64`` and 0."""
    x = torch.cos(2 * math.pi * k0 * torch.arange(N, dtype=F64) / N).float().reshape(N, 1)
    p = ops_nn.audio_spectrogram(x, N, N, magnitude_squared=True)
    assert p.shape == (1, 1, N // 2 + 1) and p.dtype == F32
    assert abs(float(p[0, 0, k0]) - N * N / 16) < 1e-3 * N * N / 16
    for k in (k0 - 1, k0 + 1):
        assert abs(float(p[0, 0, k]) - N * N / 64) < 1e-3 * N * N / 64
    rest = p[0, 0].clone()
    rest[k0 - 1:k0 + 2] = 0
    assert float(rest.max()) < 1e-6 * N * N / 16


def test_spectrogram_frames_shapes_and_the_root_form():
    x = _data(CASES[1])
    for S, window, stride, F_, bins in ((700, 200, 77, 7, 129), (199, 200, 1, 0, 129), (200, 200, 500, 1, 129),
                                        (700, 256, 256, 2, 129), (700, 257, 100, 5, 257)):
        p = ops_nn.audio_spectrogram(x[:S], window, stride, True)
        assert p.shape == (3, F_, bins), (S, window, stride, p.shape)
    p = ops_nn.audio_spectrogram(x, 200, 77, True)
    r = ops_nn.audio_spectrogram(x, 200, 77, False)
    torch.testing.assert_close(r, p.sqrt(), rtol=1e-6, atol=0)
    torch.testing.assert_close(p.to(F64), _ref(CASES[1])[0], rtol=0, atol=1e-6 * float(p.max()))
    with pytest.raises(ValueError):
        ops_nn.audio_spectrogram(x[:, 0], 200, 77)


@pytest.mark.parametrize("case", (CASES[1], CASES[4], CASES[6]), ids=_case_id)
def test_mfcc_op_is_the_plain_loop_mirror(case):
    S, B, w, st, C, D, rate, lo, hi = case
    p, m = _ref(case)
    got = ops_nn.mfcc(p, torch.tensor(rate, dtype=torch.int32), hi, lo, C, D)
    assert got.shape == (B, _frames(case), D) and got.dtype == F32
    # float64 inside, rounded to fp32 once: half an fp32 ulp of the largest coefficient
    assert float((got.to(F64) - m).abs().max()) <= 2.0 ** -24 * float(m.abs().max()) + 1e-9


def test_mfcc_of_silence():
    C, D = 40, 13
    got = ops_nn.mfcc(torch.zeros((2, 3, 257)), 16000, 4000.0, 20.0, C, D)
    assert abs(float(got[0, 0, 0]) - math.sqrt(2.0 / C) * C * math.log(1e-12)) < 1e-4
    assert float(got[..., 1:].abs().max()) < 1e-5 and torch.equal(got[0, 0], got[1, 2])


def test_mfcc_op_refusals():
    p = torch.ones((1, 2, 257))
    with pytest.raises(ValueError):
        ops_nn.mfcc(p, 16000, 4000.0, 20.0, 13, 14)                 # D > C
    with pytest.raises(ValueError):
        ops_nn.mfcc(p, 16000, 4000.0, 20.0, 200, 13)                # 200 channels over 128 bins: some are empty
    with pytest.raises(ValueError):
        ops_nn.mfcc(p[0], 16000)
    with pytest.raises(ValueError):
        K.mfcc_tables(480, 16000, 20.0, 4000.0, 200, 13)


def _wav_bytes(pcm, rate=16000, channels=1):
    bio = io.BytesIO()
    with wave.open(bio, "wb") as wf:
        wf.setnchannels(channels)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(np.asarray(pcm, dtype="<i2").tobytes())
    return bio.getvalue()


def test_decode_wav_reads_what_the_wave_module_wrote():
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, (300, 2)).astype(np.int16)
    data = _wav_bytes(pcm, rate=22050, channels=2)
    gb = GraphBuilder()
    node = gb.decode_wav(gb.placeholder("wav", "STRING", []), desired_samples=-1, name="decode")
    cut = gb.decode_wav("wav:0", desired_channels=2, desired_samples=100, name="cut")
    pad = gb.decode_wav("wav:0", desired_samples=400, name="pad")
    sess = Session(gb.build(), device=torch.device("cpu"))
    feed = {"wav:0": StringTensor(np.array([data], dtype=object).reshape(()), ())}
    audio, rate, a_cut, a_pad = sess.run([f"{node}:0", f"{node}:1", f"{cut}:0", f"{pad}:0"], feed)
    assert int(rate) == 22050 and audio.dtype == F32 and audio.shape == (300, 2)
    assert torch.equal(audio, torch.from_numpy(pcm.astype(np.float32) / 32768))
    assert torch.equal(a_cut, audio[:100]) and torch.equal(a_pad[:300], audio) and not a_pad[300:].any()
    assert a_pad.shape == (400, 2)
    for bad in (b"RIFF", data[:20], data.replace(b"WAVE", b"WAVX"), _wav8()):
        with pytest.raises(ValueError):
            ops_nn.decode_wav(bad)
    with pytest.raises(ValueError):
        ops_nn.decode_wav(data, desired_channels=1)


def _wav8():
    bio = io.BytesIO()
    with wave.open(bio, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(1)
        wf.setframerate(8000)
        wf.writeframes(bytes(range(64)))
    return bio.getvalue()


# =================================================================================== CPU: the launchers
def test_eligibility_borders():
    ok = K.mfcc_eligible
    assert ok(129, 129, 1) and ok(2048, 2048, 7) and not ok(128, 128, 1) and not ok(4096, 2049, 1)
    assert not ok(479, 480, 160) and ok(480, 480, 160) and not ok(16000, 480, 0)
    assert ok(16000, 480, 160, 40, 40, 16000, 20, 4000) and not ok(16000, 480, 160, 40, 41, 16000, 20, 4000)
    assert ok(16000, 2048, 160, 128, 1, 16000, 20, 8000) and not ok(16000, 2048, 160, 129, 13, 16000, 20, 8000)
    assert not ok(16000, 480, 160, 100, 13, 16000, 20, 4000)        # empty channels at the low end
    assert not ok(16000, 480, 160, 40, 13, None)
    assert K.audio_fft_length(129) == 256 and K.audio_fft_length(256) == 256 and K.audio_fft_length(1323) == 2048
    assert K.audio_frames(16000, 480, 160) == 98 and K.audio_frames(100, 480, 160) == 0


def test_tables():
    t = K.mfcc_tables(480, 16000, 20.0, 4000.0, 40, 13)
    assert t["fft"] == 512 and t["hann"].shape == (480,) and t["twiddle"].shape == (256, 2)
    assert t["chan"].shape == (40, 3) and t["chan"].dtype == torch.int32 and t["dct"].shape == (13, 40)
    assert float(t["hann"][0]) == 0.0 and abs(float(t["hann"][240]) - 1.0) < 1e-7
    assert torch.equal(t["twiddle"][0], torch.tensor([1.0, 0.0])) and abs(float(t["twiddle"][128, 1]) + 1.0) < 1e-7
    start, end, band, weight = _bank(257, 16000, 20.0, 4000.0, 40)
    lo, mid, hi = t["chan"][:, 0], t["chan"][:, 1], t["chan"][:, 2]
    assert int(lo[0]) == start and int(hi[-1]) <= end + 1 and bool((lo <= mid).all() and (mid <= hi).all())
    assert bool((lo[1:] == mid[:-1]).all()) and bool((mid[1:] == hi[:-1]).all())   # each bin feeds two neighbours
    for c in (0, 7, 39):
        assert [band[i] for i in range(int(mid[c]), int(hi[c]))] == [c] * int(hi[c] - mid[c])
        assert [band[i] for i in range(int(lo[c]), int(mid[c]))] == [c - 1] * int(mid[c] - lo[c])
    i = int(mid[7])
    assert abs(float(t["wa"][i]) - weight[i]) < 1e-7 and abs(float(t["wb"][i]) - (1 - weight[i])) < 1e-7
    assert K.mfcc_tables(480)["C"] == 0 and "chan" not in K.mfcc_tables(480)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_host_path_is_the_mirror(case):
    S, B, w, st, C, D, rate, lo, hi = case
    x, tb = _data(case), _tables(case)
    p, m = _ref(case)
    got = K.audio_mfcc(x, tb, st)
    assert got.shape == (B, _frames(case), D) and got.dtype == F32
    em = float((got.to(F64) - m).abs().max())
    es = max(_spec_err(K.audio_spectrogram(x, tb, st, sq), p, sq) for sq in (True, False))
    print(f"{_case_id(case)}: mfcc max err {em:g} (|m| up to {float(m.abs().max()):.1f}), spectrogram {es:g} of the peak")
    assert em < 5e-5 and es < 2e-6      # fp32 class; the measured values feed the GPU bounds


def test_measured_tolerance():
    em, es = _host_error()
    print(f"E_m = {em:g}, E_s = {es:g}; GPU bounds {8 * em:g} and {8 * es:g}")
    assert 0 < em < 5e-5 and 0 < es < 2e-6


def test_host_path_forms_agree():
    """bf16 = fp32 rounded, the padded form, ``[B, S]`` through strides, int16 with a scale."""
    case = CASES[1]
    x, tb, st = _data(case), _tables(case), case[3]
    base = K.audio_mfcc(x, tb, st)
    assert torch.equal(K.audio_mfcc(x, tb, st, out_dtype=BF), base.to(BF))
    pad = K.audio_mfcc(x, tb, st, pad8=True)
    assert pad.shape == (*base.shape, 8) and torch.equal(pad[..., 0], base.to(BF)) and not pad[..., 1:].any()
    assert torch.equal(K.audio_mfcc(x.t().contiguous().t(), tb, st), base)
    pcm = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    assert torch.equal(K.audio_mfcc(pcm, tb, st, scale=1 / 32768), K.audio_mfcc(pcm.float() * (1 / 32768), tb, st))


def test_launchers_reject_malformed_calls():
    case = CASES[1]
    x, tb, st = _data(case), _tables(case), case[3]
    with pytest.raises(ValueError):
        K.audio_mfcc(x[:, 0], tb, st)
    with pytest.raises(TypeError):
        K.audio_mfcc(x.double(), tb, st)
    with pytest.raises(ValueError):
        K.audio_mfcc(x[:100], tb, st)                               # no frame
    with pytest.raises(ValueError):
        K.audio_mfcc(x, tb, 0)
    with pytest.raises(ValueError):
        K.audio_mfcc(x, K.mfcc_tables(case[2]), st)                 # tables without a filter bank
    with pytest.raises(ValueError):
        K.audio_mfcc(x, {**tb, "wa": tb["wa"][:-1]}, st)
    with pytest.raises(TypeError):
        K.audio_mfcc(x, {**tb, "hann": tb["hann"].double()}, st)
    with pytest.raises(ValueError):
        K.audio_mfcc(x, tb, st, out=torch.empty((3, 7, 12)))
    with pytest.raises(TypeError):
        K.audio_mfcc(x, tb, st, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        K.audio_spectrogram(x, K.mfcc_tables(100), st)              # N = 128
    with pytest.raises(ValueError):
        K.audio_spectrogram(x, tb, st, out=torch.empty((3, 7, 128)))
    assert K.audio_spectrogram(x, K.mfcc_tables(case[2]), st).shape == (3, 7, 129)


FAULTS = ("frame_offset", "band_shift", "no_sqrt", "dct_no_half", "pair_swap", "window_stretch")


def test_tolerance_cannot_hide_an_indexing_bug():
    """Mirrors with one fault each against the true mirror, on the workload's case: the largest
    MFCC difference must exceed ten times the GPU bound ``8 E_m`` (about 8e-5).  Seen: frames
    offset by one sample 0.032, band shifted 7.3, no square root 16, DCT without the half 1.4, pair
    swapped 3.4, window stretched 0.62."""
    bound = _bounds()[0]
    S, B, w, st, C, D, rate, lo, hi = WORKLOAD
    x = _data(WORKLOAD).numpy()
    true = _ref(WORKLOAD)[1].numpy()
    for fault in FAULTS:
        p = _mirror_spec(x, w, st, fault=fault)
        bad = _mirror_mfcc(p, rate, lo, hi, C, D, fault=fault)
        diff = float(np.abs(bad - true).max())
        print(f"{fault}: max MFCC difference {diff:g} against a bound of {bound:g}")
        assert diff > 10 * bound, (fault, diff)


# =================================================================================== CPU: the lowering
S_, B_, W_, ST_ = 2080, 3, 480, 160
F_ = 11


def _front(gb, pcm="float32", transpose=True, scale_op="Mul", D=13):
    x = gb.placeholder("clips", "INT16" if pcm == "int16" else "FLOAT", [B_, S_] if transpose else [S_, B_])
    if pcm == "int16":
        x = gb.cast(x, "FLOAT", name="to_float")
        if scale_op == "Mul":
            x = gb.mul(x, gb.constant("scale", np.float32(1 / 32768)), name="scaled")
        elif scale_op == "RealDiv":
            x = gb.op("RealDiv", [x, gb.constant("scale", np.float32(32768))], name="scaled")
    if transpose:
        x = gb.transpose(x, [1, 0], name="samples_major")
    s = gb.audio_spectrogram(x, W_, ST_, True, name="spectrogram")
    return gb.mfcc(s, 16000, 4000.0, 20.0, 40, D, name="mfcc")


def _clips(pcm, transpose=True, seed=0):
    x = _data(WORKLOAD)[:, :B_]
    if pcm == "int16":
        x = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    return (x.t() if transpose else x).contiguous()


def _compile(gb, pcm, fetches, transpose=True, strict=True):
    spec = {"clips:0": ((B_, S_) if transpose else (S_, B_), "INT16" if pcm == "int16" else "FLOAT")}
    return gb.build(), CompiledFunction(gb.build(), spec, fetches, "cpu", strict=strict)


def _steps(plan):
    return [(s.kind, s.name.rsplit("/", 1)[-1]) for s in plan.steps]


@pytest.mark.parametrize("pcm,scale_op,transpose", (("float32", None, True), ("float32", None, False),
                                                     ("int16", "Mul", True), ("int16", "RealDiv", True),
                                                     ("int16", None, False)))
def test_lowering_absorbs_the_transpose_and_the_pcm_prefix(pcm, scale_op, transpose):
    gb = GraphBuilder()
    _front(gb, pcm, transpose, scale_op)
    g, plan = _compile(gb, pcm, ["mfcc:0"], transpose)
    assert _steps(plan) == [("mfcc", "mfcc")] and plan.summary()["glue_ops"] == []
    m = plan.steps[0].meta
    assert m["layout"] == ("clip_major" if transpose else "sample_major") and m["out"] == "fp32"   # it is fetched
    assert m["input"] == ("int16" if pcm == "int16" else "fp32")
    assert m["scale"] == (1.0 if scale_op is None else 1 / 32768)
    assert (m["S"], m["B"], m["F"], m["fft"], m["C"], m["D"]) == (S_, B_, F_, 512, 40, 13)
    x = _clips(pcm, transpose)
    got, = plan({"clips:0": x})
    want = torch.as_tensor(Session(g, device=torch.device("cpu")).run(["mfcc:0"], {"clips:0": x})[0])
    assert got.shape == (B_, F_, 13)
    scale = 32768.0 if pcm == "int16" and scale_op is None else 1.0     # unscaled PCM: the log shifts c0 only
    assert float((got - want).abs().max()) < 5e-5 * (1 + math.log(scale))


def test_lowering_writes_the_conv_input_padded():
    gb = GraphBuilder()
    m = _front(gb, "int16", D=16)
    x = gb.reshape(m, [-1, F_, 16, 1], name="fingerprint")
    w = gb.constant("w", np.random.default_rng(0).normal(0, 0.1, (3, 4, 1, 8)).astype(np.float32))
    gb.relu(gb.conv2d(x, w, name="conv"), name="out")
    g, plan = _compile(gb, "int16", ["out:0"])
    assert [s.kind for s in plan.steps] == ["mfcc", "conv"], _steps(plan)
    assert not any(s.name.endswith("/pad_cin") for s in plan.steps) and plan.summary()["glue_ops"] == []
    assert plan.steps[0].meta["out"] == "padded8" and plan.steps[0].outputs[0].phys_c == 8
    assert tuple(plan.steps[0].outputs[0].buf.shape) == (B_, F_, 16, 8)
    x = _clips("int16")
    got, = plan({"clips:0": x})
    want = torch.as_tensor(Session(g, device=torch.device("cpu")).run(["out:0"], {"clips:0": x})[0])
    # bf16 coefficients (up to ~30: half an ulp is 0.06) through 12 taps of ~0.1
    assert got.shape == want.shape and float((got - want).abs().max()) < 0.15
    # a fetched fingerprint, or a second reader, keeps the plain [B, F, D] form
    gb = GraphBuilder()
    x = gb.reshape(_front(gb, "float32", D=16), [-1, F_, 16, 1], name="fingerprint")
    gb.relu(gb.conv2d(x, gb.constant("w", np.zeros((3, 4, 1, 8), np.float32)), name="conv"), name="out")
    _, plan = _compile(gb, "float32", ["out:0", "fingerprint:0"])
    assert plan.steps[0].kind == "mfcc" and plan.steps[0].meta["out"] == "bf16"
    assert any(s.name.endswith("/pad_cin") for s in plan.steps)


@pytest.mark.parametrize("squared", (True, False))
def test_lowering_of_a_lone_spectrogram(squared):
    gb = GraphBuilder()
    x = gb.transpose(gb.placeholder("clips", "FLOAT", [B_, S_]), [1, 0], name="samples_major")
    gb.audio_spectrogram(x, W_, ST_, squared, name="spectrogram")
    g, plan = _compile(gb, "float32", ["spectrogram:0"])
    assert _steps(plan) == [("spectrogram", "spectrogram")] and plan.steps[0].meta["squared"] is squared
    x = _clips("float32")
    got, = plan({"clips:0": x})
    want = torch.as_tensor(Session(g, device=torch.device("cpu")).run(["spectrogram:0"], {"clips:0": x})[0])
    assert got.shape == (B_, F_, 257) and float(((got - want).abs().amax(-1) / want.amax(-1)).max()) < 2e-6


def _refusal(kind):
    gb = GraphBuilder()
    feeds = {"clips:0": ((B_, S_), "FLOAT")}
    fetches = ["mfcc:0"]
    if kind == "mfcc of a fed spectrogram":
        gb.mfcc(gb.placeholder("clips", "FLOAT", [B_, F_, 257]), 16000, name="mfcc")
        feeds = {"clips:0": ((B_, F_, 257), "FLOAT")}
    elif kind == "fed sample_rate":
        x = gb.transpose(gb.placeholder("clips", "FLOAT", [B_, S_]), [1, 0], name="samples_major")
        gb.mfcc(gb.audio_spectrogram(x, W_, ST_, True, name="spectrogram"), gb.placeholder("rate", "INT32", []), name="mfcc")
        feeds["rate:0"] = ((), "INT32")
    elif kind in ("window 2049", "empty channels"):
        x = gb.transpose(gb.placeholder("clips", "FLOAT", [B_, S_]), [1, 0], name="samples_major")
        s = gb.audio_spectrogram(x, 2049 if kind == "window 2049" else W_, ST_, True, name="spectrogram")
        gb.mfcc(s, 16000, 4000.0, 20.0, 100 if kind == "empty channels" else 40, 13, name="mfcc")
    elif kind == "mfcc of a second reader's spectrogram":       # the spectrogram lowers alone, the Mfcc stays
        x = gb.transpose(gb.placeholder("clips", "FLOAT", [B_, S_]), [1, 0], name="samples_major")
        gb.mfcc(gb.audio_spectrogram(x, W_, ST_, True, name="spectrogram"), 16000, name="mfcc")
        fetches = ["mfcc:0", "spectrogram:0"]
    elif kind == "transpose with a second reader":
        _front(gb)
        fetches = ["mfcc:0", "samples_major:0"]
    return gb.build(), feeds, fetches


@pytest.mark.parametrize("kind", ("mfcc of a fed spectrogram", "fed sample_rate", "window 2049", "empty channels",
                                  "mfcc of a second reader's spectrogram", "transpose with a second reader"))
def test_lowering_refusals(kind):
    g, feeds, fetches = _refusal(kind)
    with pytest.raises(CompileError):
        CompiledFunction(g, feeds, fetches, "cpu", strict=True)
    if kind in ("empty channels", "fed sample_rate"):
        # no glue plan either: the op raises on this bank, and the glue path sizes its outputs by
        # a dry run on zeros, where a sample rate of zero is no filter bank
        with pytest.raises(ValueError):
            CompiledFunction(g, feeds, fetches, "cpu")
        return
    plan = CompiledFunction(g, feeds, fetches, "cpu")
    kinds = plan.summary()["kinds"]
    assert "mfcc" not in kinds and plan.summary()["glue_ops"]
    assert ("spectrogram" in kinds) == (kind == "mfcc of a second reader's spectrogram")
    vals = {"clips:0": _clips("float32")}
    if kind == "mfcc of a fed spectrogram":
        vals = {"clips:0": _ref(WORKLOAD)[0][:B_].float()}
    want = Session(g, device=torch.device("cpu")).run(fetches, vals)
    for a, b in zip(plan(vals), want):
        # a glue step stores its fp32 result as bf16: half a bf16 ulp of coefficients up to ~32
        torch.testing.assert_close(a.float(), torch.as_tensor(b).float(), atol=0.13, rtol=0)


# =================================================================================== CPU: the model
MODEL = dict(clip_samples=2080, conv1=(5, 4, 16), conv2=(3, 4, 16), num_classes=6, top_k=3)
# the workload's filters (20 x 8 x 1 x 64 and 10 x 4 x 64 x 64, 12 classes) over an 11-frame clip: the first conv
# has 160 taps, more than the implicit GEMM takes, and runs on the direct conv in 32-channel tiles
FULL_FILTERS = dict(clip_samples=2080, num_classes=12, top_k=3)
MODELS = {"small": MODEL, "full-size filters": FULL_FILTERS}
PLAN_KINDS = ["mfcc", "conv", "pool", "conv", "gemm", "softmax_topk"]
# host plan vs fp32 interpreter, largest probability error over 4 seeds and both feeds (measured)
PLAN_ERR = {"small": 0.0041, "full-size filters": 0.0048}
# asserted on the host: twice that; the GPU plan is allowed four times


def _spotter_graph(pcm="int16", model="small"):
    from flink_tensorflow_amd.models.zoo import speech_commands_graph_def

    return Graph.from_graph_def(speech_commands_graph_def(pcm=pcm, **MODELS[model]))


def _records(n, seed=0, dtype=np.int16):
    rng = np.random.default_rng(seed)
    t = np.arange(2080) / 16000.0
    out = []
    for i in range(n):
        f = rng.uniform(200, 3000)
        a = 0.25 * rng.standard_normal(2080) + 0.4 * np.sin(2 * np.pi * f * t)
        out.append(np.clip(np.rint(a * 32768), -32768, 32767).astype(np.int16) if dtype == np.int16 else a.astype(np.float32))
    return out


@pytest.mark.parametrize("model", tuple(MODELS))
@pytest.mark.parametrize("pcm", ("int16", "float32"))
def test_host_plan_of_the_spotter_against_the_interpreter(pcm, model):
    """Strict host plan vs the fp32 interpreter: the differences are the plan's bf16 roundings (the
    coefficients, weights, activations, logits, probabilities).  Measured over 4 seeds and both
    feeds: at most 0.0041 in a probability for the small model and 0.0048 with the full-size
    filters (``PLAN_ERR``); asserted: twice that."""
    g = _spotter_graph(pcm, model)
    dt = "INT16" if pcm == "int16" else "FLOAT"
    plan = CompiledFunction(g, {"clips:0": ((4, 2080), dt)}, ["probs:0", "top_k:0", "top_k:1"], "cpu", strict=True)
    assert [s.kind for s in plan.steps] == PLAN_KINDS and plan.summary()["glue_ops"] == []
    assert not any(s.name.endswith("/pad_cin") for s in plan.steps)
    sess = Session(g, device=torch.device("cpu"))
    worst = 0.0
    for seed in range(4):
        x = torch.from_numpy(np.stack(_records(4, seed, np.int16 if pcm == "int16" else np.float32)))
        probs, vals, idxs = plan({"clips:0": x})
        ref = torch.as_tensor(sess.run(["probs:0"], {"clips:0": x})[0])
        worst = max(worst, float((probs.float() - ref).abs().max()))
        assert abs(float(probs.float().sum(-1).mean()) - 1) < 0.01
    print(f"host plan vs interpreter ({pcm}, {model}): max probability error {worst:g}")
    assert worst <= 2 * PLAN_ERR[model]


def test_conv_selector_sends_filters_past_64_taps_to_the_direct_conv():
    """The 20 x 8 first conv over one padded input channel: its bank fits LDS in 32-channel tiles
    only; what the selector chose before (``dconv`` at 64-channel tiles, else the others) is unchanged."""
    from flink_tensorflow_amd.graph.conv_lowering import ConvSite, select_conv_kernel

    def site(kernel, cin_phys=8, on_gpu=True, **kw):
        return ConvSite(on_gpu=on_gpu, x_shape=(4, 98, 40, cin_phys), cin=1, cin_phys=cin_phys, cout=64, kernel=kernel,
                        stride=(1, 1), pads=(9, 10, 3, 4), dil=(1, 1), act=K.ACT_RELU, residual=False, res_plain=False,
                        res_alias=False, **kw)

    assert not K.dconv_eligible(8, 20, 8, (1, 1), (1, 1), 2) and K.dconv_eligible(8, 20, 8, (1, 1), (1, 1), 2, 32)
    assert select_conv_kernel(site((20, 8))) == "dconv"
    assert select_conv_kernel(site((20, 8), on_gpu=False)) == "igemm"        # host plans: the reference conv
    assert select_conv_kernel(site((8, 8))) == "dconv" and K.dconv_eligible(8, 8, 8, (1, 1), (1, 1), 2)
    assert select_conv_kernel(site((40, 8))) == "igemm"                       # no kernel takes it: the launcher raises


def test_full_size_graph_has_the_documented_shapes():
    from flink_tensorflow_amd.graph.tensor_proto import tensor_from_proto
    from flink_tensorflow_amd.models.zoo import speech_commands_graph_def

    g = Graph.from_graph_def(speech_commands_graph_def())
    assert g["fingerprint/shape"].op == "Const" and g["spectrogram"].attr("window_size") == 480
    shapes = {n: tuple(int(v) for v in tensor_from_proto(g[f"{n}/shape"].attr("value")).tolist()) for n in ("fingerprint", "flatten")}
    assert shapes == {"fingerprint": (-1, 98, 40, 1), "flatten": (-1, 62720)}
    assert tuple(tensor_from_proto(g["conv1/kernel"].attr("value")).shape) == (20, 8, 1, 64)
    assert tuple(tensor_from_proto(g["conv2/kernel"].attr("value")).shape) == (10, 4, 64, 64)
    assert tuple(tensor_from_proto(g["dense/kernel"].attr("value")).shape) == (62720, 12)


def test_model_on_the_host_fallback():
    from flink_tensorflow_amd.models.zoo import KeywordSpotterModel

    recs = _records(5)
    m = KeywordSpotterModel(buckets=(8, 32), device="cpu", **MODEL)
    m.open()
    try:
        res = m.spot(recs)
        as_float = m.spot([r.astype(np.float32) / 32768 for r in recs])
        as_wav = m.spot([_wav_bytes(r) for r in recs[:2]] + [_wav_bytes(recs[2][:1000])])
        (sub, tags, _), = m.submit(recs, np.zeros(5), list(range(5)))
        assert m.poll() == [] and m.drain() == []
        with pytest.raises(ValueError):
            m.spot([recs[0][:100]])
        with pytest.raises(ValueError):
            m.spot([_wav_bytes(recs[0], rate=8000)])
    finally:
        m.close()
    assert sub == res and tags == list(range(5)) and len(res) == 5
    assert as_float == res and as_wav[:2] == res[:2] and len(as_wav) == 3     # int16 <-> float32 is exact
    sess = Session(_spotter_graph(), device=torch.device("cpu"))
    vals, idxs = sess.run(["top_k:0", "top_k:1"], {"clips:0": torch.from_numpy(np.stack(recs))})
    labels = KeywordSpotterModel().labels
    for r, v, i in zip(res, torch.as_tensor(vals).tolist(), torch.as_tensor(idxs).tolist()):
        assert r == [(p, labels[c]) for p, c in zip(v, i)]
        assert [p for p, _ in r] == sorted((p for p, _ in r), reverse=True)


def test_model_behind_map_with_model_batched():
    from flink_tensorflow_amd.models.zoo import KeywordSpotterModel
    from flink_tensorflow_amd.runtime import StreamExecutionEnvironment

    recs = _records(12, seed=3)
    env = StreamExecutionEnvironment.get_execution_environment()
    got = env.from_collection(recs).map_with_model_batched(
        KeywordSpotterModel(buckets=(8, 32), device="cpu", **MODEL), None, max_batch=8,
        max_delay_ms=1).execute_and_collect()
    ref = KeywordSpotterModel(buckets=(8, 32), device="cpu", **MODEL)
    ref.open()
    try:
        want = ref.spot(recs)
    finally:
        ref.close()
    assert len(got) == 12
    assert sorted(map(repr, got)) == sorted(map(repr, want))


def test_model_function_over_the_savedmodel(tmp_path):
    from flink_tensorflow_amd.models import PredictMethod, SavedModelModel
    from flink_tensorflow_amd.models.zoo import export_keyword_spotter_saved_model

    graph_args = {k: v for k, v in MODEL.items() if k != "top_k"}
    d = export_keyword_spotter_saved_model(str(tmp_path / "spotter"), pcm="float32", top_k=3, **graph_args)
    m = SavedModelModel(d, device="cpu")
    m.open()
    try:
        ref = m.function("serving_default", PredictMethod(), compile=False)
        fn = m.function("serving_default", PredictMethod(), compile=True, batch_buckets=None)
        x = np.stack(_records(4, seed=5, dtype=np.float32))
        a, b = ref.apply({"clips": x}), fn.apply({"clips": x})
        s = fn.plan_summary()
    finally:
        m.close()
    assert s is not None and s["glue_ops"] == [] and s["kinds"]["mfcc"] == 1
    assert b["probabilities"].shape == (4, 6) and b["classes"].shape == (4, 3)
    torch.testing.assert_close(b["probabilities"].float(), a["probabilities"].float(), atol=2 * PLAN_ERR["small"], rtol=0)


# =================================================================================== GPU: the kernel
def _banded(t, fill, dev, band=4096):
    """``t`` as a view into a larger allocation filled with ``fill`` -> (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((band + n + band,), fill, dtype=t.dtype, device=dev)
    v = buf[band:band + n].view(t.shape)
    v.copy_(t)
    return v, buf


def _bands_intact(buf, n, fill, band=4096):
    h = buf.cpu()
    lo, hi = h[:band], h[band + n:]
    if fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


_INT_FILL = {torch.int16: -32768, torch.int32: 1 << 30}


def _gpu_run(x, tb_host, stride, dev, mode="mfcc", scale=1.0, clip_major=False, **kw):
    """One launch with every operand between NaN bands (integer operands: a value that would
    wreck the result) and the output between sentinel bands -> the output on the host; the bands
    are checked here.  ``clip_major``: the samples lie ``[B, S]`` and are read through strides."""
    ops = {}
    src = x.t().contiguous() if clip_major else x
    ops["x"] = _banded(src, _INT_FILL.get(x.dtype, NAN), dev)
    tb = dict(tb_host)
    for k, v in tb_host.items():
        if isinstance(v, torch.Tensor):
            ops[k] = _banded(v, _INT_FILL.get(v.dtype, NAN), dev)
            tb[k] = ops[k][0]
    xin = ops["x"][0].t() if clip_major else ops["x"][0]
    S, B = x.shape
    F_, N = K.audio_frames(S, tb["window"], stride), tb["fft"]
    if mode == "mfcc":
        dt = kw.get("out_dtype", F32)
        shape = (B, F_, tb["D"], 8) if kw.get("pad8") else (B, F_, tb["D"])
        out, obuf = _banded(torch.full(shape, SENT, dtype=BF if kw.get("pad8") else dt), SENT, dev)
        K.audio_mfcc(xin, tb, stride, scale, out=out, **kw)
    else:
        out, obuf = _banded(torch.full((B, F_, N // 2 + 1), SENT, dtype=F32), SENT, dev)
        K.audio_spectrogram(xin, tb, stride, mode == "squared", scale, out=out)
    torch.cuda.synchronize()
    for k, (v, buf) in ops.items():
        assert _bands_intact(buf, v.numel(), _INT_FILL.get(v.dtype, NAN)), f"{k}: a guard band was written"
    assert _bands_intact(obuf, out.numel(), SENT), "out: a sentinel band was written"
    res = out.cpu()
    assert not (res.float() == SENT).any(), "an output element was not written"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_matches_the_mirror(case):
    """fp32 MFCC and both spectrogram forms of every case against the mirror, between guard bands."""
    bm, bs = _bounds()
    dev = torch.device("cuda", 0)
    x, tb, st = _data(case), _tables(case), case[3]
    p, m = _ref(case)
    got = _gpu_run(x, tb, st, dev)
    em = float((got.to(F64) - m).abs().max())
    print(f"{_case_id(case)}: mfcc max err {em:g} (allowed {bm:g})")
    assert torch.isfinite(got).all() and em <= bm
    for sq in (True, False):
        es = _spec_err(_gpu_run(x, tb, st, dev, mode="squared" if sq else "magnitude"), p, sq)
        print(f"{_case_id(case)}: spectrogram ({'squared' if sq else 'magnitude'}) err {es:g} of the peak (allowed {bs:g})")
        assert es <= bs


@pytest.mark.gpu
def test_kernel_spectrogram_of_a_tone():
    bs = _bounds()[1]
    dev = torch.device("cuda", 0)
    tb = K.mfcc_tables(WORKLOAD[2])
    for sq in (True, False):
        es = _spec_err(_gpu_run(_tone(), tb, WORKLOAD[3], dev, mode="squared" if sq else "magnitude"), _ref_tone(), sq)
        print(f"tone, {'squared' if sq else 'magnitude'}: err {es:g} of the peak (allowed {bs:g})")
        assert es <= bs


@pytest.mark.gpu
@pytest.mark.parametrize("case", SUBSET, ids=_case_id)
def test_kernel_output_forms_and_input_layouts_are_bit_equal(case):
    """bf16 = the fp32 output rounded to nearest even; the padded form = that in channel 0 and
    exact zeros in channels 1..7; ``[B, S]`` input through strides, and int16 input with a scale,
    give the bits of the plain launch; two launches give identical bits."""
    dev = torch.device("cuda", 0)
    x, tb, st = _data(case), _tables(case), case[3]
    base = _gpu_run(x, tb, st, dev)
    assert torch.equal(_gpu_run(x, tb, st, dev), base)
    assert torch.equal(_gpu_run(x, tb, st, dev, out_dtype=BF), base.to(BF))
    pad = _gpu_run(x, tb, st, dev, pad8=True)
    assert torch.equal(pad[..., 0], base.to(BF)) and not pad[..., 1:].any()
    assert torch.equal(_gpu_run(x, tb, st, dev, clip_major=True), base)
    pcm = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    scale = 1 / 32768
    as_float = _gpu_run(pcm.float() * scale, tb, st, dev)
    assert torch.equal(_gpu_run(pcm, tb, st, dev, scale=scale), as_float)
    assert torch.equal(_gpu_run(pcm, tb, st, dev, scale=scale, clip_major=True, pad8=True)[..., 0], as_float.to(BF))
    sp = _gpu_run(x, tb, st, dev, mode="squared")
    assert torch.equal(_gpu_run(x, tb, st, dev, mode="squared", clip_major=True), sp)


@pytest.mark.gpu
@pytest.mark.parametrize("case", (CASES[4], CASES[7]), ids=_case_id)
def test_kernel_clips_are_independent(case):
    """Exact: a clip's result in the batch equals the same clip run alone, in any position, and
    a silent clip among loud ones gives the silence result (``c0 = sqrt(2 / C) C ln 1e-12``)."""
    dev = torch.device("cuda", 0)
    x, tb, st = _data(case), _tables(case), case[3]
    S, B, C = case[0], case[1], case[4]
    base = _gpu_run(x, tb, st, dev)
    for b in range(B):
        assert torch.equal(_gpu_run(x[:, b:b + 1].contiguous(), tb, st, dev)[0], base[b]), f"clip {b} alone"
    mixed = torch.cat([x[:, -1:], torch.zeros((S, 1)), x[:, :1]], 1).contiguous()
    got = _gpu_run(mixed, tb, st, dev)
    assert torch.equal(got[0], base[-1]) and torch.equal(got[2], base[0])
    assert float((got[1, :, 0] - math.sqrt(2.0 / C) * C * math.log(1e-12)).abs().max()) < 1e-4
    assert float(got[1, :, 1:].abs().max()) < 1e-4 and torch.equal(got[1, 0], got[1, -1])


# =================================================================================== GPU: plan and model
@pytest.mark.gpu
@pytest.mark.parametrize("pcm,model", (("int16", "small"), ("float32", "small"), ("int16", "full-size filters")))
def test_spotter_plan_gpu(pcm, model):
    """The strict plan: ``mfcc``, conv, pool, conv, gemm, softmax / top-k; no glue op, no
    ``pad_cin`` copy.  Its probabilities against the fp32 interpreter within ``4 PLAN_ERR``."""
    dev = torch.device("cuda", 0)
    g = _spotter_graph(pcm, model)
    spec = {"clips:0": ((4, 2080), "INT16" if pcm == "int16" else "FLOAT")}
    plan = CompiledFunction(g, spec, ["probs:0", "top_k:1"], dev, strict=True)
    s = plan.summary()
    assert [st.kind for st in plan.steps] == PLAN_KINDS and s["glue_ops"] == [] and s["hip_graph"]
    assert not any(st.name.endswith("/pad_cin") for st in plan.steps)
    assert plan.steps[0].meta["out"] == "padded8" and plan.steps[0].meta["input"] == ("int16" if pcm == "int16" else "fp32")
    x = torch.from_numpy(np.stack(_records(4, 1, np.int16 if pcm == "int16" else np.float32)))
    probs, idx = plan({"clips:0": x.to(dev)})
    again = plan({"clips:0": x.to(dev)})[0]
    want, widx = Session(g, device=torch.device("cpu")).run(["probs:0", "top_k:1"], {"clips:0": x})
    want = torch.as_tensor(want).float()
    err = float((probs.float().cpu() - want).abs().max())
    print(f"{pcm}, {model}: GPU plan vs fp32 interpreter, max probability error {err:g} (allowed {4 * PLAN_ERR[model]:g})")
    assert err <= 4 * PLAN_ERR[model] and torch.equal(again.cpu(), probs.cpu())
    top2 = torch.topk(want, 2, -1).values
    assert ((idx[:, 0].cpu() == torch.as_tensor(widx)[:, 0]) | (top2[:, 0] - top2[:, 1] <= 2 * err)).all()


@pytest.mark.gpu
def test_model_gpu():
    """``spot`` and ``submit`` / ``poll`` / ``drain`` over 40 records with buckets (8, 32):
    results come back in submission order and are equal to ``spot``."""
    from flink_tensorflow_amd.models.zoo import KeywordSpotterModel

    recs = _records(40, seed=11)
    m = KeywordSpotterModel(buckets=(8, 32), **MODEL)
    m.open()
    try:
        s = m.plan_summary()
        assert s["glue_ops"] == [] and s["kinds"]["mfcc"] == 1 and s["hip_graph"]
        want = m.spot(recs)
        done = []
        for lo, hi in ((0, 32), (32, 40)):                       # buckets 32 and 8, as spot cuts them
            done += m.submit(recs[lo:hi], np.zeros(hi - lo), list(range(lo, hi)))
            done += m.poll()
        done += m.drain()
    finally:
        m.close()
    assert [t for _, tags, _ in done for t in tags] == list(range(40))
    assert [r for res, _, _ in done for r in res] == want
