// image_resize.hip -- the spectrogram image following a resize of the Spectrum editor: cpl's oglImage.resize(width / spectrumStretching,
// height, true), which Spectrum::handleFlagUpdates' resized branch runs so that the columns already on screen survive a drag of the
// editor's corner or a change of Spectrum stretch (Source/Spectrum/Spectrum.cpp:503-515).  gfx950 only.
//
// cpl's COpenGLImage::resize is not in the tree, so the rule is this library's (UNVERIFIED vs cpl; sgz.h states it).  Rows: axis point i
// sits at the same view fraction i / (P - 1) at both sizes, so new row i reads old position r = i (P0 - 1) / (P1 - 1) and blends old rows
// j = floor(r) and min(j + 1, P0 - 1) with an 8-bit weight (view_translate.hip's blend).  Columns: time stays 1:1 -- the newest
// min(C0, C1) columns keep their age relative to the write position x, which becomes x0 mod C1; older columns have no source and become
// 0x00000000, what create_image holds.
//
// The kernel gathers from a packed copy of the old image (the new image may be the old one's memory), one thread per destination texel,
// 256 contiguous bytes per wave store; the column table is a rotation, so a wave's loads are contiguous but for the one wrap.  Texels
// beyond `columns` in a wider pitch are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "runtime.hpp"

using namespace sgz;

namespace {

// grid: blocksPerRow blocks of 256 threads per new image row; row = blockIdx.x / blocksPerRow (uniform).  src [P0][C0] packed;
// rowSrc / rowWeight [P1] the table of sgz_image_resize_rows, colSrc [C1] that of sgz_image_resize_columns (-1: no source)
__global__ void __launch_bounds__(256)
imageResizeKernel(const uint32_t *src, const int32_t *rowSrc, const uint32_t *rowWeight, const int32_t *colSrc, uint8_t *image,
                  size_t pitch, uint32_t C0, uint32_t C1, uint32_t P0, uint32_t blocksPerRow)
{
    const uint32_t row = blockIdx.x / blocksPerRow;
    const uint32_t x = (blockIdx.x - row * blocksPerRow) * 256u + threadIdx.x;
    if (x >= C1) return;
    const int32_t cs = colSrc[x];
    uint32_t out = 0u;
    if (cs >= 0) {
        const uint32_t j = uint32_t(rowSrc[row]), w = rowWeight[row];
        const uint32_t a = src[size_t(j) * C0 + uint32_t(cs)];
        out = a;
        if (w) {
            const uint32_t b = src[size_t(min(j + 1u, P0 - 1u)) * C0 + uint32_t(cs)];
            out = 0u;
            for (int c = 0; c < 32; c += 8) {
                const uint32_t ac = (a >> c) & 0xffu, bc = (b >> c) & 0xffu;
                out |= ((ac * (256u - w) + bc * w + 128u) >> 8) << c;
            }
        }
    }
    *reinterpret_cast<uint32_t *>(image + size_t(row) * pitch + size_t(x) * 4) = out;
}

bool validAxis(uint32_t P) { return P >= 2 && P <= (1u << 20); }

}  // namespace

namespace sgz {

bool validAxisPoints(uint32_t P) { return validAxis(P); }

bool validImageLayout(const void *d_image, uint32_t columns, size_t pitch)
{
    return columns > 0 && pitch >= size_t(columns) * 4 && !(pitch & 3) && !(reinterpret_cast<uintptr_t>(d_image) & 3);
}

// the tables of sgz_image_resize_rows / sgz_image_resize_columns (arguments checked by the caller)
void imageResizeRows(uint32_t P0, uint32_t P1, int32_t *src, uint16_t *weight)
{
#pragma clang fp contract(off)
    const double last0 = P0 - 1.0, last1 = P1 - 1.0;
    for (uint32_t i = 0; i < P1; ++i) {
        const double r = (double(i) * last0) / last1;
        double j = std::floor(r);
        double w = std::floor((r - j) * 256.0 + 0.5);
        if (w == 256.0) { j += 1.0; w = 0.0; }
        src[i] = int32_t(j);
        weight[i] = uint16_t(w);
    }
}

uint32_t imageResizeColumns(uint32_t C0, uint32_t x0, uint32_t C1, int32_t *src)
{
    const uint32_t x1 = x0 % C1, keep = std::min(C0, C1);
    for (uint32_t c = 0; c < C1; ++c) {
        const uint64_t age = (uint64_t(x1) + C1 - 1u - c) % C1;       // (x1 - 1 - c) mod C1
        src[c] = age < keep ? int32_t((uint64_t(x0) + C0 - 1u - age) % C0) : -1;
    }
    return x1;
}

bool imageResizeFits(uint32_t C0, uint32_t C1, uint32_t P1)
{
    return (uint64_t(C1) + 255u) / 256u * P1 <= 0x7fffffffu && C0 <= 0x7fffffffu && C1 <= 0x7fffffffu;
}

size_t imageResizeScratchFloats(uint32_t P0, uint32_t C0, uint32_t P1, uint32_t C1)
{
    return size_t(P1) * 2 + size_t(C1) + size_t(P0) * C0;
}

// the old image (device, [P0][srcPitch], next write column x0) resampled into the new one ([P1][dstPitch]); the two may share memory.
// `scratch` / `scratchCap` (floats) hold the tables and the packed copy of the old image the kernel gathers from (grown here).  Waits
// for the result.
sgz_status resizeImage(const uint8_t *src, uint32_t C0, size_t srcPitch, uint32_t P0, uint32_t x0, uint8_t *dst, uint32_t C1,
                       size_t dstPitch, uint32_t P1, uint32_t *x1, float **scratch, size_t *scratchCap, hipStream_t stream)
{
    if (!imageResizeFits(C0, C1, P1)) return fail(SGZ_EINVAL, "image resize: more than 2^31 workgroups or columns");
    const uint64_t blocksPerRow = (uint64_t(C1) + 255u) / 256u, blocks = blocksPerRow * P1;
    std::vector<int32_t> rowSrc(P1), colSrc(C1);
    std::vector<uint16_t> w16(P1);
    imageResizeRows(P0, P1, rowSrc.data(), w16.data());
    const uint32_t newX = imageResizeColumns(C0, x0, C1, colSrc.data());
    const std::vector<uint32_t> rowWeight(w16.begin(), w16.end());
    // scratch: row src [P1] int32 | row weights [P1] uint32 | column src [C1] int32 | the old image's texels [P0][C0]
    if (sgz_status st = ensureCap(scratch, scratchCap, imageResizeScratchFloats(P0, C0, P1, C1)); st != SGZ_OK) return st;
    int32_t *d_rows = reinterpret_cast<int32_t *>(*scratch);
    uint32_t *d_w = reinterpret_cast<uint32_t *>(d_rows + P1);
    int32_t *d_cols = reinterpret_cast<int32_t *>(d_w + P1);
    uint32_t *d_copy = reinterpret_cast<uint32_t *>(d_cols + C1);
    SGZ_HIP(hipMemcpyAsync(d_rows, rowSrc.data(), size_t(P1) * 4, hipMemcpyHostToDevice, stream));
    SGZ_HIP(hipMemcpyAsync(d_w, rowWeight.data(), size_t(P1) * 4, hipMemcpyHostToDevice, stream));
    SGZ_HIP(hipMemcpyAsync(d_cols, colSrc.data(), size_t(C1) * 4, hipMemcpyHostToDevice, stream));
    SGZ_HIP(hipMemcpy2DAsync(d_copy, size_t(C0) * 4, src, srcPitch, size_t(C0) * 4, P0, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(imageResizeKernel, dim3(unsigned(blocks)), dim3(256), 0, stream, d_copy, d_rows, d_w, d_cols, dst, dstPitch, C0, C1,
                       P0, uint32_t(blocksPerRow));
    SGZ_HIP(hipGetLastError());
    SGZ_HIP(hipStreamSynchronize(stream));                   // (the host tables are read by the copies above)
    if (x1) *x1 = newX;
    return SGZ_OK;
}

}  // namespace sgz

extern "C" {

sgz_status sgz_image_resize_rows(uint32_t old_axis_points, uint32_t new_axis_points, int32_t *src, uint16_t *weight)
{
    if (!src || !weight) return fail(SGZ_EINVAL, "null argument");
    if (!validAxis(old_axis_points) || !validAxis(new_axis_points)) return fail(SGZ_EINVAL, "2 <= axis_points <= 2^20");
    imageResizeRows(old_axis_points, new_axis_points, src, weight);
    return SGZ_OK;
}

sgz_status sgz_image_resize_columns(uint32_t old_columns, uint32_t old_x, uint32_t new_columns, int32_t *src, uint32_t *new_x)
{
    if (!src || !new_x) return fail(SGZ_EINVAL, "null argument");
    if (old_columns == 0 || new_columns == 0 || old_columns > 0x7fffffffu || new_columns > 0x7fffffffu) return fail(SGZ_EINVAL, "0 < columns < 2^31");
    if (old_x >= old_columns) return fail(SGZ_EINVAL, "old_x < old_columns");
    *new_x = imageResizeColumns(old_columns, old_x, new_columns, src);
    return SGZ_OK;
}

sgz_status sgz_image_resize_device(const void *d_src, uint32_t old_columns, size_t src_pitch_bytes, uint32_t old_axis_points, uint32_t old_x,
                                   void *d_dst, uint32_t new_columns, size_t dst_pitch_bytes, uint32_t new_axis_points, uint32_t *new_x,
                                   void *stream)
{
    if (!d_src || !d_dst) return fail(SGZ_EINVAL, "null argument");
    if (!validAxis(old_axis_points) || !validAxis(new_axis_points)) return fail(SGZ_EINVAL, "2 <= axis_points <= 2^20");
    if (!validImageLayout(d_src, old_columns, src_pitch_bytes) || !validImageLayout(d_dst, new_columns, dst_pitch_bytes))
        return fail(SGZ_EINVAL, "image: columns > 0, pitch >= 4 * columns, 4-byte aligned");
    if (old_x >= old_columns) return fail(SGZ_EINVAL, "old_x < old_columns");
    // the bytes each image spans: [base, base + pitch (P - 1) + 4 columns)
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    const uintptr_t s1 = s0 + src_pitch_bytes * (old_axis_points - 1u) + size_t(old_columns) * 4;
    const uintptr_t d1 = d0 + dst_pitch_bytes * (new_axis_points - 1u) + size_t(new_columns) * 4;
    if (s0 < d1 && d0 < s1) return fail(SGZ_EINVAL, "source and destination images overlap");
    float *scratch = nullptr; size_t cap = 0;
    const sgz_status st = resizeImage(static_cast<const uint8_t *>(d_src), old_columns, src_pitch_bytes, old_axis_points, old_x,
                                      static_cast<uint8_t *>(d_dst), new_columns, dst_pitch_bytes, new_axis_points, new_x, &scratch, &cap,
                                      reinterpret_cast<hipStream_t>(stream));
    if (scratch) {
        (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
        (void)hipFree(scratch);
    }
    return st;
}

}  // extern "C"
