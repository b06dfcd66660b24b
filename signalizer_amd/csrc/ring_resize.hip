// ring_resize.hip -- the real-time Spectrum's mirrored audio ring at a new capacity, keeping its newest samples: what a change of the
// window size, of the hop under RSNT or of the algorithm needs (sgz_spectrum_update; the ring's capacity is (RSNT ? hop : W) + 2 pieces,
// realtime.hip).  cpl's AudioStream history resize is not in the tree, so the rule is this library's (UNVERIFIED vs cpl; sgz.h states it).
// gfx950 only.
//
// The ring of one channel holds every sample twice, at p and p + cap, with p = t mod cap for absolute sample t; `written` samples have
// gone in.  The new ring holds, for every t in [written - new_cap, written), at t mod new_cap and t mod new_cap + new_cap (non-negative
// residues): the old sample when t >= written - old_cap and t >= 0, otherwise 0 -- silence, as a ring starts.  `written` itself does not
// change, so every position derived from it (ringPos) stays valid.
//
// One thread per (channel, new slot), taken in the order of t: the L = min(old_cap, new_cap, written) samples that move are one
// contiguous range of the old (mirrored) ring, read with consecutive addresses by consecutive lanes; both mirror stores come from the
// same lane and are consecutive too, but for the one wrap of the new ring.  A one-off copy per update, not a per-frame path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "runtime.hpp"

using namespace sgz;

namespace {

// grid: (ceil(newCap / 256), channels).  Thread i is t = written - newCap + i: zero below iFirst = newCap - L, otherwise old ring
// position oldBase + (i - iFirst) (< 2 oldCap: the mirror); new ring position newBase + i mod newCap (newBase = written mod newCap).
__global__ void __launch_bounds__(256)
ringResizeKernel(const float *oldRing, uint32_t oldCap, float *newRing, uint32_t newCap, uint32_t oldBase, uint32_t newBase, uint32_t iFirst)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y;
    if (i >= newCap) return;
    const float v = i >= iFirst ? oldRing[size_t(c) * 2 * oldCap + oldBase + (i - iFirst)] : 0.f;
    uint32_t p = newBase + i;
    if (p >= newCap) p -= newCap;
    float *r = newRing + size_t(c) * 2 * newCap;
    r[p] = v;
    r[p + newCap] = v;
}

bool overlaps(const void *a, size_t aBytes, const void *b, size_t bBytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bBytes && y < x + aBytes;
}

}  // namespace

namespace sgz {

bool validRingResize(const float *d_old, uint32_t oldCap, const float *d_new, uint32_t newCap, uint32_t channels)
{
    if (!d_old || !d_new || oldCap == 0 || newCap == 0 || channels == 0 || channels > 65535u) return false;
    if (oldCap > 0x7fffffffu || newCap > 0x7fffffffu) return false;              // (2 cap in 32 bits)
    return !overlaps(d_old, size_t(channels) * 2 * oldCap * sizeof(float), d_new, size_t(channels) * 2 * newCap * sizeof(float));
}

// enqueues the move on `stream` (arguments checked by the caller: validRingResize); nothing is waited for
sgz_status resizeRing(const float *d_old, uint32_t oldCap, float *d_new, uint32_t newCap, uint32_t channels, uint64_t written, hipStream_t stream)
{
    const uint64_t L = std::min<uint64_t>(std::min(oldCap, newCap), written);
    const uint32_t oldBase = uint32_t((written % oldCap + oldCap - L) % oldCap);
    const uint32_t newBase = uint32_t(written % newCap);
    const uint32_t iFirst = newCap - uint32_t(L);
    hipLaunchKernelGGL(ringResizeKernel, dim3((newCap + 255u) / 256u, channels), dim3(256), 0, stream, d_old, oldCap, d_new, newCap, oldBase,
                       newBase, iFirst);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz

extern "C" {

sgz_status sgz_ring_resize_device(const float *d_old, uint32_t old_cap, float *d_new, uint32_t new_cap, uint32_t channels, uint64_t written,
                                  void *stream)
{
    if (!validRingResize(d_old, old_cap, d_new, new_cap, channels))
        return fail(SGZ_EINVAL, "ring resize: non-null rings, 0 < capacity < 2^31, 1 <= channels <= 65535, rings that do not overlap");
    return resizeRing(d_old, old_cap, d_new, new_cap, channels, written, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
