// line_graph.hip -- the Spectrum line graph's vertex stream (DisplayMode::LineGraph, the reference's default view): what
// Spectrum::renderTransformAsGraph (Source/Spectrum/SpectrumRendering.cpp:794-897) hands PrimitiveDrawer::addVertex for every pair,
// built in HBM from the handle's line results instead of one addVertex at a time on the CPU.  gfx950 only.
//
// Per pair (one renderTransformAsGraph call each, :639-652), S = 2 sides for Separate / MidSide / Phase (the fall-throughs at :831,
// :877), 1 for the other modes; graph k runs 1, 0 ("back to front"), the right side before the left one:
//   flood fill (alphaFloodFill != 0, :807): per (k, side) 2P vertices, GL_LINES: (i, y, z), (i, endPoint, z)
//   strips:                                 per (k, side)  P vertices, GL_LINE_STRIP: (i, y, z)
// y = results[i].second (right side, z = -0.5) or .first (left side, z = 0); endPoint = 0 (dbs.high > dbs.low always holds: the plan
// refuses high_db <= low_db and getDBs() only widens the range).  The model matrix (translate, scale) is GL state: sgz_line_graph_draws
// hands its coefficients to the host with the draw list, colours and line widths.  Host arithmetic only there; the kernel is a pure
// store stream (no LDS, no scratch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "runtime.hpp"

using namespace sgz;

namespace {

// GL_LINES / GL_LINE_STRIP, the primitive types renderTransformAsGraph opens its PrimitiveDrawers with
static_assert(SGZ_PRIM_LINES == 0x0001u && SGZ_PRIM_LINE_STRIP == 0x0003u, "the GL enumerants");

inline uint32_t lineGraphSides(uint32_t mode)
{
    return (mode == SGZ_CH_SEPARATE || mode == SGZ_CH_MIDSIDE || mode == SGZ_CH_PHASE) ? 2u : 1u;
}

// juce ColourHelpers::floatToUInt8 (juce_Colour.cpp:27-30): the alpha byte of withAlpha(float)
inline uint8_t floatToUInt8(float a) { return a <= 0.0f ? 0 : (a >= 1.0f ? 255 : static_cast<uint8_t>(a * 255.996f)); }

struct LineGraphParams {
    const float2 *lines;            // [pairs][SGZ_NUM_GRAPHS][P] (.x = first / left, .y = second / right)
    float3 *xyz;                    // [pairs][vertices per pair]
    uint32_t P, sides, blocksPerRow, flood;
};

// grid: blocksPerRow blocks of 256 threads per row; row = pair * (graphs * sides) + block, block = the (k, side) position in draw order
// (k = 1 first, right before left).  Thread i of a row reads results[i] once and stores its strip vertex and, with the flood fill on,
// the two fill vertices: a wave's stores are 768 (strip) and 1536 (fill) contiguous bytes.
__global__ void __launch_bounds__(256) lineGraphVertexKernel(const LineGraphParams prm)
{
    const uint32_t row = blockIdx.x / prm.blocksPerRow;                       // (uniform: scalar)
    const uint32_t i = (blockIdx.x - row * prm.blocksPerRow) * 256u + threadIdx.x;
    if (i >= prm.P) return;
    const uint32_t S = prm.sides, perPairBlocks = SGZ_NUM_GRAPHS * S;
    const uint32_t pair = row / perPairBlocks, b = row - pair * perPairBlocks;
    const uint32_t k = (SGZ_NUM_GRAPHS - 1) - b / S;
    const bool right = S == 2 && (b % S) == 0;
    const float2 r = prm.lines[(size_t(pair) * SGZ_NUM_GRAPHS + k) * prm.P + i];
    const float x = float(i), y = right ? r.y : r.x, z = right ? -0.5f : 0.0f;
    const size_t P = prm.P, blockVerts = size_t(perPairBlocks) * P;
    float3 *base = prm.xyz + size_t(pair) * blockVerts * (prm.flood ? 3u : 1u);
    if (prm.flood) {
        float3 *fill = base + size_t(b) * 2 * P + 2 * size_t(i);
        fill[0] = make_float3(x, y, z);
        fill[1] = make_float3(x, 0.0f, z);                                    // endPoint
        base += 2 * blockVerts;                                               // the strips follow every fill of the pair
    }
    base[size_t(b) * P + i] = make_float3(x, y, z);
}

}  // namespace

namespace sgz {
// the launch behind sgz_line_graph_vertices_device (also the handle's, realtime.hip); arguments checked by the caller
sgz_status launchLineGraphVertices(const float *d_lines, uint32_t pairs, uint32_t P, uint32_t mode, uint32_t flood, float *d_xyz,
                                   hipStream_t stream)
{
    LineGraphParams prm{};
    prm.lines = reinterpret_cast<const float2 *>(d_lines);
    prm.xyz = reinterpret_cast<float3 *>(d_xyz);
    prm.P = P; prm.sides = lineGraphSides(mode); prm.flood = flood ? 1u : 0u;
    prm.blocksPerRow = (P + 255u) / 256u;
    const uint64_t blocks = uint64_t(prm.blocksPerRow) * pairs * SGZ_NUM_GRAPHS * prm.sides;
    if (blocks > 0x7fffffffu) return fail(SGZ_EINVAL, "line graph: more than 2^31 workgroups");
    hipLaunchKernelGGL(lineGraphVertexKernel, dim3(unsigned(blocks)), dim3(256), 0, stream, prm);
    SGZ_HIP(hipGetLastError());
    return SGZ_OK;
}
}  // namespace sgz

extern "C" {

size_t sgz_line_graph_vertex_count(uint32_t channel_mode, uint32_t pairs, uint32_t axis_points, uint32_t flood)
{
    if (channel_mode > SGZ_CH_COMPLEX) return 0;
    return size_t(pairs) * SGZ_NUM_GRAPHS * lineGraphSides(channel_mode) * axis_points * (flood ? 3u : 1u);
}

sgz_status sgz_line_graph_draws(const sgz_line_graph_style *style, uint32_t channel_mode, uint32_t pairs, uint32_t axis_points,
                                sgz_line_graph_draw *out, uint32_t *count, float model[4])
{
    if (!style || !count) return fail(SGZ_EINVAL, "null argument");
    if (channel_mode > SGZ_CH_COMPLEX || pairs == 0 || axis_points == 0) return fail(SGZ_EINVAL, "channel mode, pairs or axis points out of range");
    const uint32_t S = lineGraphSides(channel_mode), flood = style->flood_alpha != 0.0f ? 1u : 0u;    // :807
    const uint64_t need = uint64_t(pairs) * SGZ_NUM_GRAPHS * S * (flood + 1);
    if (need > 0xffffffffu || sgz_line_graph_vertex_count(channel_mode, pairs, axis_points, flood) > 0xffffffffu)
        return fail(SGZ_EINVAL, "line graph: more than 2^32 vertices or draws");
    if (*count < need || !out) { *count = uint32_t(need); return fail(SGZ_EINVAL, "draw list too small (count holds the required size)"); }
    const float fillWidth = static_cast<float>(style->rendering_scale);                                            // :797
    const float stripWidth = std::max(0.001f, static_cast<float>(style->rendering_scale * style->primitive_size));   // :852
    const uint8_t fillAlpha = floatToUInt8(style->flood_alpha);                                                      // withAlpha(float)
    const uint32_t P = axis_points, perPair = SGZ_NUM_GRAPHS * S * P * (flood ? 3u : 1u);
    uint32_t n = 0;
    for (uint32_t p = 0; p < pairs; ++p) {
        uint32_t first = p * perPair;
        for (uint32_t strip = flood ? 0u : 1u; strip < 2; ++strip)             // fills (:807-848), then strips (:850-896)
            for (int k = SGZ_NUM_GRAPHS - 1; k >= 0; --k)
                for (uint32_t side = S; side-- > 0;) {                          // right (1), then left (0)
                    const uint8_t *base = side ? style->colour_two[k] : style->colour_one[k];
                    sgz_line_graph_draw &d = out[n++];
                    d.first = first;
                    d.count = strip ? P : 2 * P;
                    d.primitive = strip ? SGZ_PRIM_LINE_STRIP : SGZ_PRIM_LINES;
                    d.pair = p; d.graph = uint32_t(k); d.side = side;
                    // ColourRotation(colour, pairs, false)[p] = withRotatedHue(float(p) / float(pairs)): RGB through HSB, alpha kept
                    rotateHueRgb8(base, float(p) / float(pairs), d.rgba);
                    d.rgba[3] = strip ? base[3] : fillAlpha;
                    d.line_width = strip ? stripWidth : fillWidth;
                    first += d.count;
                }
    }
    *count = n;
    if (model) {                                                                // :801-802: translate(-1, -1, 0), then scale
        model[0] = static_cast<float>(1.0 / (double(P - 1) * 0.5));
        model[1] = 2.0f;
        model[2] = -1.0f;
        model[3] = -1.0f;
    }
    return SGZ_OK;
}

sgz_status sgz_line_graph_vertices_device(const float *d_lines, uint32_t pairs, uint32_t axis_points, uint32_t channel_mode,
                                          uint32_t flood, float *d_xyz, void *stream)
{
    if (!d_lines || !d_xyz) return fail(SGZ_EINVAL, "null argument");
    if (channel_mode > SGZ_CH_COMPLEX) return fail(SGZ_EINVAL, "channel mode out of range");
    if (axis_points > (1u << 24)) return fail(SGZ_EINVAL, "axis points above 2^24 (x = (float) i stays exact below)");
    if (pairs == 0 || axis_points == 0) return SGZ_OK;
    return launchLineGraphVertices(d_lines, pairs, axis_points, channel_mode, flood, d_xyz, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
