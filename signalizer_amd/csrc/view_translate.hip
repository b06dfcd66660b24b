// view_translate.hip -- the spectrogram image following a change of view: cpl's oglImage.freeLinearVerticalTranslation(oldViewRect,
// state.viewRect), which Spectrum::handleFlagUpdates' viewChanged branch runs in colour-spectrum mode (Source/Spectrum/Spectrum.cpp:560-561)
// so that the columns already on screen follow a zoom or a pan.  gfx950 only.
//
// Image row y is axis point y (columnScatterKernel, realtime.hip), and axis point i sits at view fraction left + (right - left) i / (P - 1)
// in every scaling and channel mode (remapFrequencies): a translation in view-fraction space maps whole rows.  cpl's resampling is not in
// the tree, so the rule is this library's (UNVERIFIED vs cpl; sgz.h states it): new row i reads old position
//     r = (new_left + S1 * (i / (P - 1)) - old_left) / S0 * (P - 1)              (S0, S1: the old and new view widths; fp64)
// and blends old rows j = floor(r) and min(j + 1, P - 1) with an 8-bit weight; rows whose r lies outside [-0.5, P - 0.5] have no source
// and become 0x00000000, what create_image holds.
//
// The kernel gathers from a copy of the image (the translation is in place: a row may read rows the same launch rewrites), one thread
// per texel, 256 contiguous bytes per wave load and store.  Texels beyond `columns` in a wider pitch are not touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "runtime.hpp"

using namespace sgz;

namespace {

// grid: blocksPerRow blocks of 256 threads per image row; row = blockIdx.x / blocksPerRow (uniform).  src [P][columns] packed,
// rowSrc / rowWeight [P] the table of sgz_view_translation_rows.
__global__ void __launch_bounds__(256)
viewTranslateKernel(const uint32_t *src, const int32_t *rowSrc, const uint32_t *rowWeight, uint8_t *image, size_t pitch, uint32_t columns,
                    uint32_t P, uint32_t blocksPerRow)
{
    const uint32_t row = blockIdx.x / blocksPerRow;
    const uint32_t x = (blockIdx.x - row * blocksPerRow) * 256u + threadIdx.x;
    if (x >= columns) return;
    const int32_t j = rowSrc[row];
    uint32_t out = 0u;
    if (j >= 0) {
        const uint32_t w = rowWeight[row];
        const uint32_t a = src[size_t(j) * columns + x];
        out = a;
        if (w) {
            const uint32_t b = src[size_t(min(uint32_t(j) + 1u, P - 1u)) * columns + x];
            out = 0u;
            for (int c = 0; c < 32; c += 8) {
                const uint32_t ac = (a >> c) & 0xffu, bc = (b >> c) & 0xffu;
                out |= ((ac * (256u - w) + bc * w + 128u) >> 8) << c;
            }
        }
    }
    *reinterpret_cast<uint32_t *>(image + size_t(row) * pitch + size_t(x) * 4) = out;
}

bool validView(double l, double r) { return std::isfinite(l) && std::isfinite(r) && l >= 0.0 && r <= 1.0 && r > l; }

}  // namespace

namespace sgz {

bool validViewRect(double left, double right) { return validView(left, right); }

// the table of sgz_view_translation_rows (arguments checked by the caller)
void viewTranslationRows(uint32_t P, double oldLeft, double oldRight, double newLeft, double newRight, int32_t *src, uint16_t *weight)
{
#pragma clang fp contract(off)
    const double S0 = oldRight - oldLeft, S1 = newRight - newLeft, last = P - 1.0;
    for (uint32_t i = 0; i < P; ++i) {
        const double u = newLeft + S1 * (double(i) / last);
        double r = (u - oldLeft) / S0 * last;
        if (!(r >= -0.5 && r <= double(P) - 0.5)) { src[i] = -1; weight[i] = 0; continue; }
        r = std::min(std::max(r, 0.0), last);
        double j = std::floor(r);
        double w = std::floor((r - j) * 256.0 + 0.5);
        if (w == 256.0) { j += 1.0; w = 0.0; }
        src[i] = int32_t(j);
        weight[i] = uint16_t(w);
    }
}

// the translation of a P x columns RGBA8 image in DEVICE memory, in place; `scratch` / `scratchCap` (floats) hold the table and the copy of
// the image it gathers from (grown here).  Waits for the result.
sgz_status translateViewImage(uint8_t *image, uint32_t columns, size_t pitch, uint32_t P, const double oldView[2], const double newView[2],
                              float **scratch, size_t *scratchCap, hipStream_t stream)
{
    const uint64_t blocksPerRow = (uint64_t(columns) + 255u) / 256u, blocks = blocksPerRow * P;
    if (blocks > 0x7fffffffu) return fail(SGZ_EINVAL, "view translation: more than 2^31 workgroups");
    std::vector<int32_t> rowSrc(P);
    std::vector<uint16_t> w16(P);
    viewTranslationRows(P, oldView[0], oldView[1], newView[0], newView[1], rowSrc.data(), w16.data());
    const std::vector<uint32_t> rowWeight(w16.begin(), w16.end());
    // scratch: src rows [P] int32 | weights [P] uint32 | the image's texels [P][columns]
    if (sgz_status st = ensureCap(scratch, scratchCap, size_t(P) * 2 + size_t(P) * columns); st != SGZ_OK) return st;
    int32_t *d_src = reinterpret_cast<int32_t *>(*scratch);
    uint32_t *d_w = reinterpret_cast<uint32_t *>(*scratch) + P;
    uint32_t *d_copy = d_w + P;
    SGZ_HIP(hipMemcpyAsync(d_src, rowSrc.data(), size_t(P) * 4, hipMemcpyHostToDevice, stream));
    SGZ_HIP(hipMemcpyAsync(d_w, rowWeight.data(), size_t(P) * 4, hipMemcpyHostToDevice, stream));
    SGZ_HIP(hipMemcpy2DAsync(d_copy, size_t(columns) * 4, image, pitch, size_t(columns) * 4, P, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(viewTranslateKernel, dim3(unsigned(blocks)), dim3(256), 0, stream, d_copy, d_src, d_w, image, pitch, columns, P,
                       uint32_t(blocksPerRow));
    SGZ_HIP(hipGetLastError());
    SGZ_HIP(hipStreamSynchronize(stream));                   // (the host tables are read by the copies above)
    return SGZ_OK;
}

}  // namespace sgz

extern "C" {

sgz_status sgz_view_translation_rows(uint32_t axis_points, double old_left, double old_right, double new_left, double new_right,
                                     int32_t *src, uint16_t *weight)
{
    if (!src || !weight) return fail(SGZ_EINVAL, "null argument");
    if (axis_points < 2) return fail(SGZ_EINVAL, "axis_points >= 2");
    if (!validView(old_left, old_right) || !validView(new_left, new_right)) return fail(SGZ_EINVAL, "view must satisfy 0 <= left < right <= 1");
    viewTranslationRows(axis_points, old_left, old_right, new_left, new_right, src, weight);
    return SGZ_OK;
}

sgz_status sgz_view_translate_device(void *d_image, uint32_t columns, size_t pitch_bytes, uint32_t axis_points, double old_left,
                                     double old_right, double new_left, double new_right, void *stream)
{
    if (!d_image) return fail(SGZ_EINVAL, "null argument");
    if (axis_points < 2 || axis_points > (1u << 20)) return fail(SGZ_EINVAL, "2 <= axis_points <= 2^20");
    if (columns == 0 || pitch_bytes < size_t(columns) * 4 || (pitch_bytes & 3) || (reinterpret_cast<uintptr_t>(d_image) & 3))
        return fail(SGZ_EINVAL, "image: columns > 0, pitch >= 4 * columns, 4-byte aligned");
    if (!validView(old_left, old_right) || !validView(new_left, new_right)) return fail(SGZ_EINVAL, "view must satisfy 0 <= left < right <= 1");
    const double oldView[2] = {old_left, old_right}, newView[2] = {new_left, new_right};
    float *scratch = nullptr; size_t cap = 0;
    const sgz_status st = translateViewImage(static_cast<uint8_t *>(d_image), columns, pitch_bytes, axis_points, oldView, newView, &scratch,
                                             &cap, reinterpret_cast<hipStream_t>(stream));
    if (scratch) {
        (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
        (void)hipFree(scratch);
    }
    return st;
}

}  // extern "C"
