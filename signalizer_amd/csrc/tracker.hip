// tracker.hip -- the frequency tracker's peak search over the raw transform: the raw-FFT branch of
// Spectrum::drawFrequencyTracking, Source/Spectrum/SpectrumRendering.cpp:379-469.  gfx950 only.
//   nearest peak of |source|^2 inside the +-3 % neighbourhood of the mouse position (std::max_element: the FIRST largest), the walk
//   along a still rising edge when the peak sits on a boundary of the range (:400-427), then the parabolic fit through the three dB
//   values around it (:431-444) -> bin, fractional bin, frequency, dB.
// One workgroup: the range is at most a few thousand bins; the reduction key is (square, smaller index wins), i.e. max_element's.
// The batched forms (one workgroup of 256 per record, nothing allocated, nothing waited for): trackPeaksKernel, the same search over
// [records][N + 1] bins, and trackLinePeaksKernel, the line-results branch (:300-377, trackPeakLines below restated) over the line
// results of a whole render, with trackValuePeaksKernel, the same body (trackLineRecord) over [records][P] value planes -- the kept peaks
// of an overview or a view.  Their boundary walks are cooperative: a wave tests 256 neighbour pairs per step and takes the first hit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "runtime.hpp"

#pragma clang fp contract(off)

using namespace sgz;

namespace {

// the parabolic fit through the three dB values around `peak` (:431-444) and the record; one thread
__device__ __forceinline__ void fitPeak(const float *bins, long peak, uint32_t N, float invSize, double sampleRate, sgz_peak *out)
{
    const long ia = peak == 0 ? 0 : peak - 1, ic = peak == long(N) ? peak : peak + 1;
    const float alpha = 20 * log10f(fabsf(bins[ia] * invSize));
    const float beta = 20 * log10f(fabsf(bins[peak] * invSize));
    const float gamma = 20 * log10f(fabsf(bins[ic] * invSize));
    const double phi = 0.5 * (alpha - gamma) / (alpha - 2 * beta + gamma);
    auto isNormal = [](double v) { const double a = fabs(v); return a >= 2.2250738585072014e-308 && a < INFINITY; };
    const double peakFraction = 2 * (double(peak) + (isNormal(phi) ? phi : 0)) / double(N);
    double peakDBs = beta - 0.25 * (alpha - gamma) * phi;
    if (!isNormal(peakDBs)) peakDBs = 20 * log10(double(fabsf(bins[peak])) / (double(N) * 0.5));
    out->peak_offset = double(peak); out->peak_fraction = peakFraction; out->peak_frequency = 0.5 * peakFraction * sampleRate;
    out->peak_dbs = peakDBs; out->alpha = alpha; out->beta = beta; out->gamma = gamma; out->phi = phi;
}

__global__ void __launch_bounds__(1024)
trackPeakKernel(const float *bins, uint32_t N, long lower, long higher, float invSize, double sampleRate, sgz_peak *out)
{
    __shared__ float sSq[16];
    __shared__ long sIdx[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto sqOf = [&](long k) { const float m = bins[k]; return m * m + 0.f; };         // Math::square(complex) with imag == 0
    float best = -1.f;
    long arg = higher + 1;
    for (long k = lower + tid; k <= higher; k += blockDim.x) {
        const float s = sqOf(k);
        if (s > best) { best = s; arg = k; }                    // ascending k per thread: its first largest (a NaN square never wins)
    }
    // max_element's order over the whole range: larger square, then the smaller index
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const long oa = __shfl_xor(arg, o);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) { sSq[wave] = best; sIdx[wave] = arg; }
    __syncthreads();
    if (tid != 0) return;
    for (unsigned w = 1; w < blockDim.x / 64; ++w)
        if (sSq[w] > best || (sSq[w] == best && sIdx[w] < arg)) { best = sSq[w]; arg = sIdx[w]; }
    long peak = arg > higher ? lower : arg;                     // (all squares NaN: max_element keeps the first element)
    if (peak == lower && lower != 0) {                          // :400-413
        for (;;) {
            const long next = peak - 1;
            if (next == 0) break;
            else if (sqOf(next) < sqOf(peak)) break;
            else peak = next;
        }
    } else if (peak == higher - 1) {                            // :414-427
        for (;;) {
            const long next = peak + 1;
            if (next == long(N)) break;
            else if (sqOf(next) < sqOf(peak)) break;
            else peak = next;
        }
    }
    fitPeak(bins, peak, N, invSize, sampleRate, out);
}

// ---- the batched forms ----
constexpr int kTrackThreads = 256;       // one workgroup per record
constexpr int kWalkUnroll = 4;           // neighbour pairs a lane tests per step of a walk: 64 lanes x 4 = 256 candidates, loads independent

// A boundary walk (:400-427 / :320-345) is a pure neighbour predicate: walking from `from` in direction `dir` it stops at the first k whose
// `hit(k)` holds.  One wave tests 256 candidates k = from + dir c per step, ballots, and takes the first hit.  `count` candidates exist (the
// last one hits by the walk's own end-of-axis stop), so nothing outside the record is read.  Every lane returns the same k.
template <typename Hit>
__device__ __forceinline__ long walkFirstHit(long from, long count, int dir, int lane, Hit hit)
{
    for (long c0 = 0; c0 < count; c0 += 64 * kWalkUnroll) {
        unsigned long long m[kWalkUnroll];
#pragma unroll
        for (int j = 0; j < kWalkUnroll; ++j) {
            const long c = c0 + j * 64 + lane;
            m[j] = __ballot(c < count && hit(from + dir * c));
        }
#pragma unroll
        for (int j = 0; j < kWalkUnroll; ++j)
            if (m[j]) return from + dir * (c0 + j * 64 + (__ffsll(m[j]) - 1));
    }
    return count > 0 ? from + dir * (count - 1) : from;
}

// trackPeakKernel over [records][N + 1] bins: the same search (square, smaller index wins; a NaN square never wins), the same walks as
// first hits, the same fit
__global__ void __launch_bounds__(kTrackThreads)
trackPeaksKernel(const float *allBins, uint32_t N, long lower, long higher, float invSize, double sampleRate, sgz_peak *out)
{
    __shared__ float sSq[kTrackThreads / 64];
    __shared__ long sIdx[kTrackThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *bins = allBins + size_t(blockIdx.x) * (size_t(N) + 1);
    auto sqOf = [&](long k) { const float m = bins[k]; return m * m + 0.f; };
    float best = -1.f;
    long arg = higher + 1;
    for (long k = lower + tid; k <= higher; k += kTrackThreads) {
        const float s = sqOf(k);
        if (s > best) { best = s; arg = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const long oa = __shfl_xor(arg, o);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) { sSq[wave] = best; sIdx[wave] = arg; }
    __syncthreads();
    if (wave != 0) return;
    best = sSq[0]; arg = sIdx[0];
    for (int w = 1; w < kTrackThreads / 64; ++w)
        if (sSq[w] > best || (sSq[w] == best && sIdx[w] < arg)) { best = sSq[w]; arg = sIdx[w]; }
    long peak = arg > higher ? lower : arg;
    if (peak == lower && lower != 0)                            // :400-413: the largest k <= peak with k - 1 == 0 or sq(k - 1) < sq(k)
        peak = walkFirstHit(peak, peak, -1, lane, [&](long k) { return k - 1 == 0 || sqOf(k - 1) < sqOf(k); });
    else if (peak == higher - 1)                                // :414-427: the smallest k >= peak with k + 1 == N or sq(k + 1) < sq(k)
        peak = walkFirstHit(peak, long(N) - peak, 1, lane, [&](long k) { return k + 1 == long(N) || sqOf(k + 1) < sqOf(k); });
    if (lane == 0) fitPeak(bins, peak, N, invSize, sampleRate, out + blockIdx.x);
}

// what trackPeakLines derives from the plan and the mouse position alone, formed on the host as it forms them
struct LineTrackParams {
    long points, lowerBound, higherBound, axisLast;
    double lowDb, dbRange, devianceFloor;
    int floorApplies;
};

// trackPeakLines (below) for one record, by one workgroup: `left(i)` reads the searched value of axis point i, wherever the record keeps it;
// lane 0 of wave 0 writes *o.  What trackLinePeaksKernel and trackValuePeaksKernel share
template <typename Left>
__device__ __forceinline__ void trackLineRecord(Left left, const LineTrackParams &prm, const float *mapped, const float *slopeMap, sgz_line_peak *o)
{
    __shared__ float sVal[kTrackThreads / 64];
    __shared__ long sIdx[kTrackThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long N = prm.points;
    // the host loop "if (left(peak) < left(i)) peak = i" from left(start): the first largest; a NaN never wins, a NaN at the start stays
    // (every comparison with it is false) -- both fall out of the same comparisons here
    float best = left(prm.lowerBound < N ? prm.lowerBound : N - 1);
    long arg = prm.lowerBound < N ? prm.lowerBound : N - 1;
    for (long i = prm.lowerBound + 1 + tid; i < prm.higherBound; i += kTrackThreads) {
        const float v = left(i);
        if (best < v) { best = v; arg = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const long oa = __shfl_xor(arg, o);
        if (best < ob || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) { sVal[wave] = best; sIdx[wave] = arg; }
    __syncthreads();
    if (wave != 0) return;
    best = sVal[0]; arg = sIdx[0];
    for (int w = 1; w < kTrackThreads / 64; ++w)
        if (best < sVal[w] || (sVal[w] == best && sIdx[w] < arg)) { best = sVal[w]; arg = sIdx[w]; }
    long peak = arg;
    if (peak == prm.lowerBound && prm.lowerBound != 0)                                                    // :320-332
        peak = walkFirstHit(peak, peak, -1, lane, [&](long k) { return k - 1 == 0 || left(k - 1) < left(k); });
    else if (prm.higherBound != 0 && peak == prm.higherBound - 1)                                         // :333-345
        peak = walkFirstHit(peak, N - peak, 1, lane, [&](long k) { return k + 1 == N || left(k + 1) < left(k); });
    if (lane != 0) return;
    const bool offsetIsEnd = peak == prm.axisLast;
    const long hi = offsetIsEnd ? peak : peak + 1, lo = offsetIsEnd ? (peak == 0 ? 0 : peak - 1) : peak;
    double peakDeviance = double(mapped[hi] - mapped[lo]);
    if (prm.floorApplies) peakDeviance = peakDeviance < prm.devianceFloor ? prm.devianceFloor : peakDeviance;      // std::max   :355-358
    const float y = left(peak);
    o->peak_offset = double(peak);
    o->peak_frequency = double(mapped[peak]);
    o->peak_deviance = peakDeviance;
    o->peak_fraction_y = double(y);
    o->peak_dbs = prm.lowDb + double(y) * prm.dbRange;           // one multiply, one add (fp contract off: no fused form)
    o->peak_slope = double(slopeMap[peak]);
}

// per record of [records][graphs][P] float2 line results: record r searches graph `graph`, first components
__global__ void __launch_bounds__(kTrackThreads)
trackLinePeaksKernel(const float *lines, uint32_t graph, const LineTrackParams prm, const float *mapped, const float *slopeMap, sgz_line_peak *out)
{
    const float *results = lines + ((size_t(blockIdx.x) * SGZ_NUM_GRAPHS + graph) * size_t(prm.points)) * 2;
    trackLineRecord([&](long i) { return results[2 * i]; }, prm, mapped, slopeMap, out + blockIdx.x);
}

// per record of [records][P] float values -- the planes V / V' every overview and view call writes: record r searches values[r]
__global__ void __launch_bounds__(kTrackThreads)
trackValuePeaksKernel(const float *values, const LineTrackParams prm, const float *mapped, const float *slopeMap, sgz_line_peak *out)
{
    const float *record = values + size_t(blockIdx.x) * size_t(prm.points);
    trackLineRecord([&](long i) { return record[i]; }, prm, mapped, slopeMap, out + blockIdx.x);
}

// the line-results branch's search range (:305-312) from the clamped mouse position
struct LineRange { size_t lowerBound, higherBound; };
LineRange lineSearchRange(size_t N, double mouseFraction)
{
    const double nearbyFractionToConsider = 0.03;
    const size_t pivot = size_t(std::llround(double(N) * mouseFraction));
    const size_t range = size_t(std::llround(double(N) * nearbyFractionToConsider));
    return {range > pivot ? 0 : pivot - range, range + pivot > N ? N : range + pivot};
}

// the raw-FFT branch's refusals and the bounds of its search range from the mouse position (:383-392)
sgz_status trackPeakBounds(const Plan &p, double mouseFraction, long &lower, long &higher)
{
    if (p.cfg.channel_mode == SGZ_CH_PHASE || p.cfg.channel_mode == SGZ_CH_COMPLEX)
        return fail(SGZ_EUNSUPPORTED, "frequency tracker: raw-FFT branch of the non-Complex magnitude modes (SpectrumRendering.cpp:301)");
    if (!std::isfinite(mouseFraction)) return fail(SGZ_EINVAL, "mouse_fraction");
    mouseFraction = mouseFraction < 0 ? 0 : (mouseFraction > 1 ? 1 : mouseFraction);                      // :292
    const double nearby = 0.03, sampleRate = double(p.cfg.sample_rate);
    const long points = long(p.P), N = long(p.N);
    auto confine = [](long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); };
    lower = std::llround(double(points) * (mouseFraction - nearby));
    lower = std::llround(double(float(size_t(N)) * p.mapped[size_t(confine(lower, 0, points - 1))]) / sampleRate);
    higher = std::llround(double(points) * (mouseFraction + nearby));
    higher = std::llround(double(float(size_t(N)) * p.mapped[size_t(confine(higher, 0, points - 1))]) / sampleRate);
    lower = confine(lower, 0, N); higher = confine(higher, 0, N);
    return SGZ_OK;
}

}  // namespace

namespace sgz {

// the search range, then the kernel; d_out: DEVICE sgz_peak
sgz_status runTrackPeak(const Plan &p, const float *d_bins, double mouseFraction, sgz_peak *d_out, hipStream_t stream)
{
    long lower = 0, higher = 0;
    if (sgz_status st = trackPeakBounds(p, mouseFraction, lower, higher); st != SGZ_OK) return st;
    hipLaunchKernelGGL(trackPeakKernel, dim3(1), dim3(1024), 0, stream, d_bins, p.N, lower, higher, p.scalars.invSize, double(p.cfg.sample_rate), d_out);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// runTrackPeak for every record of d_bins [records][N + 1] in one launch; d_out: DEVICE sgz_peak [records]
sgz_status runTrackPeaks(const Plan &p, const float *d_bins, size_t records, double mouseFraction, sgz_peak *d_out, hipStream_t stream)
{
    long lower = 0, higher = 0;
    if (sgz_status st = trackPeakBounds(p, mouseFraction, lower, higher); st != SGZ_OK) return st;
    if (records == 0) return SGZ_OK;
    if (records > 0x7fffffffu) return fail(SGZ_EINVAL, "too many records for one launch");
    hipLaunchKernelGGL(trackPeaksKernel, dim3(unsigned(records)), dim3(kTrackThreads), 0, stream, d_bins, p.N, lower, higher, p.scalars.invSize,
                       double(p.cfg.sample_rate), d_out);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// what both line-results launches share: the clamp (:292), the search range and the plan's constants.  The entry points have checked a
// finite mouseFraction and uploaded the plan's tables.
static sgz_status lineTrackParams(const Plan &p, size_t records, double mouseFraction, LineTrackParams &prm)
{
    mouseFraction = mouseFraction < 0 ? 0 : (mouseFraction > 1 ? 1 : mouseFraction);                      // :292
    const size_t N = p.P;
    if (N == 0) return fail(SGZ_EINVAL, "no axis points");
    if (records > 0x7fffffffu) return fail(SGZ_EINVAL, "too many records for one launch");
    if (!p.d_mappedFreq || !p.d_slope) return fail(SGZ_EINVAL, "plan tables not uploaded");
    const LineRange r = lineSearchRange(N, mouseFraction);
    prm = LineTrackParams{};
    prm.points = long(N); prm.lowerBound = long(r.lowerBound); prm.higherBound = long(r.higherBound);
    prm.axisLast = long(size_t(p.cfg.axis_points) - 1);
    prm.lowDb = p.cfg.low_db; prm.dbRange = p.cfg.high_db - p.cfg.low_db;
    prm.floorApplies = p.cfg.algorithm == SGZ_ALGO_FFT && p.cfg.bin_interp != SGZ_INTERP_LANCZOS;
    prm.devianceFloor = 0.5 * double(p.N) / double(N);
    return SGZ_OK;
}

// trackPeakLines for every (frame, pair) of d_lines [frames][pairs][graphs][P] float2 in one launch; d_out: DEVICE sgz_line_peak
// [frames][pairs].  The entry points have checked graph < SGZ_NUM_GRAPHS and a finite mouseFraction and uploaded the plan's tables.
sgz_status runTrackPeaksLines(const Plan &p, const float *d_lines, size_t frames, uint32_t graph, double mouseFraction, sgz_line_peak *d_out,
                              hipStream_t stream)
{
    if (p.P == 0) return fail(SGZ_EINVAL, "no axis points");
    if (frames == 0) return SGZ_OK;
    if (frames > 0x7fffffffu / p.C) return fail(SGZ_EINVAL, "too many (frame, pair) records for one launch");
    LineTrackParams prm{};
    if (sgz_status st = lineTrackParams(p, frames * p.C, mouseFraction, prm); st != SGZ_OK) return st;
    hipLaunchKernelGGL(trackLinePeaksKernel, dim3(unsigned(frames * p.C)), dim3(kTrackThreads), 0, stream, d_lines, graph, prm, p.d_mappedFreq,
                       p.d_slope, d_out);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

// the same for every record of d_values [records][P] float in one launch; d_out: DEVICE sgz_line_peak [records]
sgz_status runTrackPeaksValues(const Plan &p, const float *d_values, size_t records, double mouseFraction, sgz_line_peak *d_out, hipStream_t stream)
{
    if (p.P == 0) return fail(SGZ_EINVAL, "no axis points");
    if (records == 0) return SGZ_OK;
    LineTrackParams prm{};
    if (sgz_status st = lineTrackParams(p, records, mouseFraction, prm); st != SGZ_OK) return st;
    hipLaunchKernelGGL(trackValuePeaksKernel, dim3(unsigned(records)), dim3(kTrackThreads), 0, stream, d_values, prm, p.d_mappedFreq, p.d_slope, d_out);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}

}  // namespace sgz

namespace sgz {

// The tracker's line-results branch (SpectrumRendering.cpp:300-377), host arithmetic on host-resident results (see sgz.h).
// `stride`: floats from one axis point's searched value to the next -- 2 for float2 line results (the first component), 1 for a value plane.
static sgz_status trackPeakStrided(const Plan &p, const float *results, size_t stride, double mouseFraction, sgz_line_peak *out)
{
    if (!std::isfinite(mouseFraction)) return fail(SGZ_EINVAL, "mouse_fraction");
    mouseFraction = mouseFraction < 0 ? 0 : (mouseFraction > 1 ? 1 : mouseFraction);                      // :292
    const size_t N = p.P;                                                                                 // results.size()
    if (N == 0) return fail(SGZ_EINVAL, "no axis points");
    auto left = [&](size_t i) { return results[stride * i]; };                                            // UComplex::leftMagnitude
    const LineRange r = lineSearchRange(N, mouseFraction);
    const size_t lowerBound = r.lowerBound, higherBound = r.higherBound;
    // std::max_element over [lowerBound, higherBound): the first largest (an empty range -- fewer than 17 axis points -- yields its own
    // begin in the reference; confined to the last point here so that nothing is read behind the results)
    size_t peak = lowerBound < N ? lowerBound : N - 1;
    for (size_t i = lowerBound + 1; i < higherBound; ++i)
        if (left(peak) < left(i)) peak = i;
    if (peak == lowerBound && lowerBound != 0) {                                                          // :320-332
        for (;;) {
            const size_t next = peak - 1;
            if (next == 0) break;
            else if (left(next) < left(peak)) break;
            else peak = next;
        }
    } else if (higherBound != 0 && peak == higherBound - 1) {                                             // :333-345
        for (;;) {
            const size_t next = peak + 1;
            if (next == N) break;
            else if (left(next) < left(peak)) break;
            else peak = next;
        }
    }
    const size_t peakOffset = peak;
    const bool offsetIsEnd = peakOffset == size_t(p.cfg.axis_points) - 1;
    // mapFrequency returns T = float: the difference is a float subtraction (TransformConstant.h:99-102)
    const size_t hi = offsetIsEnd ? peakOffset : peakOffset + 1, lo = offsetIsEnd ? (peakOffset == 0 ? 0 : peakOffset - 1) : peakOffset;
    double peakDeviance = double(p.mapped[hi] - p.mapped[lo]);
    if (p.cfg.algorithm == SGZ_ALGO_FFT && p.cfg.bin_interp != SGZ_INTERP_LANCZOS)
        peakDeviance = std::max(peakDeviance, 0.5 * double(p.N) / double(N));                             // :355-358
    out->peak_offset = double(peakOffset);
    out->peak_frequency = double(p.mapped[peakOffset]);
    out->peak_deviance = peakDeviance;
    out->peak_fraction_y = double(left(peakOffset));
    out->peak_dbs = p.cfg.low_db + double(left(peakOffset)) * (p.cfg.high_db - p.cfg.low_db);
    out->peak_slope = double(p.slope[peakOffset]);
    return SGZ_OK;
}

sgz_status trackPeakLines(const Plan &p, const float *results, double mouseFraction, sgz_line_peak *out)
{
    return trackPeakStrided(p, results, 2, mouseFraction, out);
}

sgz_status trackPeakValues(const Plan &p, const float *values, double mouseFraction, sgz_line_peak *out)
{
    return trackPeakStrided(p, values, 1, mouseFraction, out);
}

}  // namespace sgz

struct sgz_plan { Plan impl; };

extern "C" sgz_status sgz_track_peak_lines(const sgz_plan *plan, const float *results, double mouse_fraction, sgz_line_peak *out)
{
    if (!plan || !results || !out) return fail(SGZ_EINVAL, "null argument");
    return trackPeakLines(plan->impl, results, mouse_fraction, out);
}

extern "C" sgz_status sgz_track_peak_values(const sgz_plan *plan, const float *values, double mouse_fraction, sgz_line_peak *out)
{
    if (!plan || !values || !out) return fail(SGZ_EINVAL, "null argument");
    return trackPeakValues(plan->impl, values, mouse_fraction, out);
}

extern "C" sgz_status sgz_stage_track_peak(sgz_plan *plan, const float *d_bins, double mouse_fraction, sgz_peak *out, void *stream)
{
    if (!plan || !d_bins || !out) return fail(SGZ_EINVAL, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    sgz_peak *d_out = nullptr;
    SGZ_HIP(hipMalloc(reinterpret_cast<void **>(&d_out), sizeof(sgz_peak)));
    sgz_status st = runTrackPeak(plan->impl, d_bins, mouse_fraction, d_out, s);
    hipError_t e = hipSuccess;
    if (st == SGZ_OK) {
        e = hipMemcpyAsync(out, d_out, sizeof(sgz_peak), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    (void)hipFree(d_out);
    if (st != SGZ_OK) return st;
    if (e != hipSuccess) return hipFail(e, "sgz_stage_track_peak");
    return SGZ_OK;
}

extern "C" sgz_status sgz_stage_track_peaks(sgz_plan *plan, const float *d_bins, size_t records, double mouse_fraction, sgz_peak *d_out, void *stream)
{
    if (!plan || !d_bins || !d_out) return fail(SGZ_EINVAL, "null argument");
    return runTrackPeaks(plan->impl, d_bins, records, mouse_fraction, d_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" sgz_status sgz_stage_track_peaks_lines(sgz_plan *plan, const float *d_lines, size_t frames, uint32_t graph, double mouse_fraction,
                                                  sgz_line_peak *d_out, void *stream)
{
    if (!plan || !d_lines || !d_out) return fail(SGZ_EINVAL, "null argument");
    if (graph >= SGZ_NUM_GRAPHS) return fail(SGZ_EINVAL, "graph");
    if (!std::isfinite(mouse_fraction)) return fail(SGZ_EINVAL, "mouse_fraction");
    if (frames == 0) return SGZ_OK;
    Plan &p = plan->impl;
    if (!p.uploaded) {                                           // the kernel reads the plan's device tables
        std::string err;
        const sgz_status st = uploadPlan(p, err);
        if (st != SGZ_OK) return fail(st, err);
    }
    return runTrackPeaksLines(p, d_lines, frames, graph, mouse_fraction, d_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" sgz_status sgz_stage_track_peaks_values(sgz_plan *plan, const float *d_values, size_t records, double mouse_fraction, sgz_line_peak *d_out,
                                                   void *stream)
{
    if (!plan || !d_values || !d_out) return fail(SGZ_EINVAL, "null argument");
    if (!std::isfinite(mouse_fraction)) return fail(SGZ_EINVAL, "mouse_fraction");
    if (records == 0) return SGZ_OK;
    Plan &p = plan->impl;
    if (!p.uploaded) {                                           // the kernel reads the plan's device tables
        std::string err;
        const sgz_status st = uploadPlan(p, err);
        if (st != SGZ_OK) return fail(st, err);
    }
    return runTrackPeaksValues(p, d_values, records, mouse_fraction, d_out, reinterpret_cast<hipStream_t>(stream));
}
