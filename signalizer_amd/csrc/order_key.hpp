// order_key.hpp -- the total order on floats that the overview (overview.hip) and the waveform lane (wave_columns.hip) reduce under: NaNs
// take no part, the others compare by the key  bits ^ (sign ? 0xFFFFFFFF : 0x80000000)  as unsigned, i.e. IEEE order with -0 below +0.  A
// greatest (or least) key is associative and commutative, so any split of the work gives the same bits, and a key turns back into the value's
// own bits.
//   the maximum   key 0 is "no value yet": it is the key of a NaN pattern (0xFFFFFFFF) and of nothing else -- -inf's key is 0x007FFFFF
//   the minimum   kept as key - 1, so that 0xFFFFFFFF is "no value yet": a NaN's key 0 wraps to it (a NaN's key must never reach a minimum as
//                 0), and no value's key is 0 -- the keys of values are 0x007FFFFF (-inf) .. 0xFF800000 (+inf), on which key - 1 keeps the order
// A group of NaNs alone turns back into 0x7FC00000 either way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgz {

__host__ __device__ __forceinline__ uint32_t orderKey(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0u;                          // a NaN takes no part
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}
__host__ __device__ __forceinline__ uint32_t keyBits(uint32_t key)
{
    if (key == 0u) return 0x7fc00000u;                                          // nothing but NaNs
    return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu);
}

__host__ __device__ __forceinline__ uint32_t orderKeyMin(uint32_t bits) { return orderKey(bits) - 1u; }
__host__ __device__ __forceinline__ uint32_t keyBitsMin(uint32_t keyMin) { return keyBits(keyMin + 1u); }

}  // namespace sgz
