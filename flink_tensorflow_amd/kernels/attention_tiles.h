// LDS tile helpers shared by the attention kernels (attention.hip, attention_causal.hip):
// head dim 64, K rows chunk-swizzled for conflict-free b128 fragment reads, V and P^T read
// through the hardware transpose read as MFMA operands.
#pragma once
#include "common.h"

namespace attn {

constexpr int D = 64;       // head dim
constexpr int VP = D + 8;   // V row pitch (elements): tr-read rows land on distinct banks
constexpr int OP = D + 8;   // output staging row pitch
constexpr int QP = 16 + 4;  // P^T row pitch: [key][16 q] tiles, 40-B rows (tr-read friendly)

typedef short v4s __attribute__((ext_vector_type(4)));

FTM_DEVICE int kswz(int row, int chunk) { return row * D + ((chunk ^ (row & 7)) << 3); }

// 4 consecutive keys x 1 d column per lane (a 16-lane group reads 4 keys x 16 d columns)
FTM_DEVICE v4s tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p);
}

// two transposed reads 4 rows apart -> one 8-element MFMA operand (whole-vector
// reinterpretation: element-wise short->bf16 inserts miscompile here)
FTM_DEVICE bf16x8 tr_read8(const bf16* p, int pitch) {
  const v4s lo = tr_read(p), hi = tr_read(p + 4 * pitch);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace attn
