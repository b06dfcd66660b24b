// scope_ring.hpp -- what the Oscilloscope's vertex kernels share (scope_vector.hip: the Linear / Rectangular / Lanczos strips of
// drawWavePlot; scope_dense.hip: the per-column min / max reduction of the Linear strip): the evaluator, the ring's index arithmetic,
// the extent of the Linear strip of a frame, and the stream-ordered scratch of the stage calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/sgz.h"

namespace sgz {

// ---- drawWavePlot on the handle's front ring (sgz_scope_vertices): the ring's write cursor is read from device memory, the
// sample comes from an evaluator (SampleColourEvaluators.h: one channel, or 0.5 (l +- r)), and a vertex is (x, y, 0) + RGBA8.
__device__ __forceinline__ float evalSample(const float *a, const float *b, uint32_t mode, uint32_t idx)
{
    if (mode == 1u) return 0.5f * (a[idx] + b[idx]);       // MidSideEvaluatorBase<0, std::plus<>>::evaluateSample
    if (mode == 2u) return 0.5f * (a[idx] - b[idx]);       // <1, std::minus<>>
    return a[idx];
}

// The reference's ring of `len` samples inside a physical ring of `cap` >= len (Spectral mode keeps the largest ring the reference can
// ask for, see sgz.h): logical position q (counted from the write cursor = the oldest of the newest `len` samples) -> memory index.
// cap == len (every other mode): (cursor + q) mod len, the ring itself.
__device__ __forceinline__ uint32_t ringPhys(long rel, uint32_t cursor, uint32_t cap, uint32_t len)
{
    long q = rel % long(len);
    if (q < 0) q += long(len);
    return uint32_t((long(cursor) + long(cap - len) + q) % long(cap));
}

// ringPhys(rel + k * step, ..) for k = 0, 1, 2, ..: the two 64-bit modulos (~100 instructions each) once, in ringPhys itself, then steps
// with a wrap -- the same indices.  The logical ring is the `len` positions from `lead` on (mod cap); q is the position inside it.
struct RingWalk {
    uint32_t lead, q, len, cap, stepMod, phys;
    __device__ __forceinline__ RingWalk(long rel, uint32_t step, uint32_t cursor, uint32_t cap_, uint32_t len_) : len(len_), cap(cap_)
    {
        phys = ringPhys(rel, cursor, cap, len);
        lead = cursor % cap + (cap - len);                 // ringPhys(0, ..) without its 64-bit modulos
        if (lead >= cap) lead -= cap;
        q = phys >= lead ? phys - lead : phys + (cap - lead);
        stepMod = step % len;
    }
    __device__ __forceinline__ void next()
    {
        q += stepMod;
        if (q >= len) q -= len;
        phys = lead + q;
        if (phys >= cap) phys -= cap;
    }
};

// The Linear strip of a frame (OscilloscopeRendering.cpp:588-631): vertex i reads logical sample  i - bufferOffset,  i < n =
// endCondition = max(2, ceil(window)) + quantizedCycleSamples
struct LinearExtent { size_t n; long bufferOffset; };
inline LinearExtent scopeLinearExtent(double windowSize, uint32_t triggerMode, double cycleSamples, long long transport)
{
    const long roundedWindow = long(std::ceil(windowSize));
    long bufferOffset, quantizedCycleSamples = 0;
    if (triggerMode == SGZ_TRIG_WINDOW) {
        bufferOffset = long(std::ceil(std::fmod(double(transport), windowSize)));   // :588-592
    } else if (triggerMode == SGZ_TRIG_ZERO_CROSSING || triggerMode == SGZ_TRIG_ENVELOPE_HOLD) {
        const double realOffset = (windowSize * 0.5 - double(int(windowSize * 0.5))) - 1.5;
        bufferOffset = long(std::ceil(realOffset));                                 // :593-594
    } else {
        // :598-612; this branch is never Lanczos, so cycleBuffers = 1
        if (triggerMode == SGZ_TRIG_SPECTRAL) quantizedCycleSamples = long(std::ceil(cycleSamples));
        bufferOffset = roundedWindow + quantizedCycleSamples;
    }
    return LinearExtent{size_t(std::max<long>(2, roundedWindow) + quantizedCycleSamples), bufferOffset};
}

// Scratch of the stage calls: stream-ordered allocations (hipMallocAsync / hipFreeAsync on the caller's stream), so the library keeps
// no process-wide device state -- any number of host threads, streams and devices may use the stage calls at once.
struct StreamScratch {
    void *p = nullptr;
    hipStream_t s;
    explicit StreamScratch(hipStream_t stream) : s(stream) {}
    hipError_t get(size_t bytes) { return hipMallocAsync(&p, bytes, s); }
    ~StreamScratch() { if (p) (void)hipFreeAsync(p, s); }
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
};

}  // namespace sgz
