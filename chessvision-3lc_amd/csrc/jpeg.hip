// jpeg.hip -- the device half of the JPEG decoder: everything after the Huffman stage (jpeg.cpp), for gfx950.
//
//   jpeg_idct_kernel    dequantise + the "islow" integer inverse DCT of libjpeg (jidctint: 13-bit constants, 2 extra bits after the
//                       column pass, columns then rows, all int32), + 128, saturated to a byte.  Quantised coefficients in,
//                       component planes of bytes out (padded to whole MCUs, row stride = 8 * blocks per row).
//   jpeg_colour_kernel  libjpeg's fancy (triangle) chroma up-sampling for 2x1 and 2x2 luma sampling, with its edge rules taken on
//                       the component's TRUE down-sampled size, then the 16-bit fixed-point YCbCr -> RGB conversion.  Planes in,
//                       interleaved BGR / RGB / gray pixels out.
//   jpeg_colour_oriented_kernel  the same colour stage storing the picture as its EXIF orientation tag (2..8) turns it: the mirror,
//                       rotation or transposition happens in an LDS tile between the per-lane work and stores along output rows.
//
// All arithmetic is wrapping 32-bit (unsigned adds and multiplies, arithmetic right shifts), so the kernels and the numpy form
// (chessvision/jpeg.py: reconstruct) agree on ANY coefficients, not only on those an encoder writes.  Every address is a function of
// the geometry alone: no coefficient value reaches an index.
//
// A wave takes eight blocks.  Lane (block, j) loads row j of its block with one 16-byte load, dequantises it and puts it into LDS;
// lane (block, c) then runs the column pass on column c, the result goes back through LDS, and lane (block, r) runs the row pass on
// row r and stores its eight bytes.  A block occupies 72 words of LDS, rows 9 words apart: with 64 banks both the row-wise and the
// column-wise accesses of a wave are conflict-free (bank = 8 * block + 9 * row + column mod 64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_device.h"

namespace cv {

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct JpegGeom {
    int ncomp, width, height, hs, vs;
    int blocks_w[3], blocks_h[3];
    unsigned block_off[3];                 // first block of each component in an image's coefficient buffer
    unsigned blocks;                       // blocks per image = bytes of planes per image / 64
    unsigned plane_off[3];                 // byte offset of each component plane in an image's planes
};

// one 8-point pass of jidctint.c's jpeg_idct_islow; `shift` = 11 after the column pass, 18 after the row pass
__device__ __forceinline__ void idct8(const uint32_t* in, int shift, int32_t* out) {
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u;
    uint32_t tmp3 = z1 + z2 * 6270u;
    z2 = in[0]; z3 = in[4];
    uint32_t tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u; z3 = 0u - z3 * 16069u; z4 = 0u - z4 * 3196u;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const uint32_t rnd = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + tmp3 + rnd) >> shift;
    out[7] = (int32_t)(tmp10 - tmp3 + rnd) >> shift;
    out[1] = (int32_t)(tmp11 + tmp2 + rnd) >> shift;
    out[6] = (int32_t)(tmp11 - tmp2 + rnd) >> shift;
    out[2] = (int32_t)(tmp12 + tmp1 + rnd) >> shift;
    out[5] = (int32_t)(tmp12 - tmp1 + rnd) >> shift;
    out[3] = (int32_t)(tmp13 + tmp0 + rnd) >> shift;
    out[4] = (int32_t)(tmp13 - tmp0 + rnd) >> shift;
}

constexpr int kBlocksPerGroup = 32;        // 256 lanes, 8 per block
constexpr int kBlockWords = 72;

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coeffs, const uint16_t* __restrict__ qtables,
                                                        uint8_t* __restrict__ planes, JpegGeom g, size_t total_blocks) {
    __shared__ uint32_t lds[kBlocksPerGroup * kBlockWords];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const size_t gb = (size_t)blockIdx.x * kBlocksPerGroup + lb;
    const bool live = gb < total_blocks;                         // every lane reaches both barriers
    const size_t img = live ? gb / g.blocks : 0;
    const unsigned b = live ? (unsigned)(gb - img * g.blocks) : 0u;
    const int c = (g.ncomp == 3 && b >= g.block_off[1]) ? (b >= g.block_off[2] ? 2 : 1) : 0;
    uint32_t* mine = lds + lb * kBlockWords;
    if (live) {
        const u32x4 cv4 = *reinterpret_cast<const u32x4*>(coeffs + gb * 64 + j * 8);
        const u32x4 qv4 = *reinterpret_cast<const u32x4*>(qtables + (img * g.ncomp + c) * 64 + j * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int32_t cf = (int16_t)(cv4[k >> 1] >> ((k & 1) * 16));
            const uint32_t q = (qv4[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
            mine[j * 9 + k] = (uint32_t)cf * q;
        }
    }
    __syncthreads();
    uint32_t in[8];
    int32_t out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = mine[r * 9 + j];         // column j
    idct8(in, 11, out);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) mine[r * 9 + j] = (uint32_t)out[r];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = mine[j * 9 + k];         // row j
    idct8(in, 18, out);
    if (!live) return;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int32_t v = out[k] + 128;
        const uint32_t px = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        if (k < 4) lo |= px << (8 * k); else hi |= px << (8 * (k - 4));
    }
    const unsigned bc = b - g.block_off[c];
    const unsigned br = bc / (unsigned)g.blocks_w[c], bx = bc % (unsigned)g.blocks_w[c];
    uint8_t* d = planes + img * ((size_t)g.blocks * 64) + g.plane_off[c] + ((size_t)br * 8 + j) * ((size_t)g.blocks_w[c] * 8) + (size_t)bx * 8;
    *reinterpret_cast<u32x2*>(d) = u32x2{lo, hi};
}

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// The per-lane work of the colour stage, shared by both colour kernels: the four adjacent pixels x0 .. x0 + 3 (x0 a multiple of 4, below
// the width) of row y of the image whose planes start at `base`.  Fancy up-sampling with its edge rules, then the fixed-point
// conversion; px[3 i .. 3 i + 2] is pixel i in the channel order asked for (B, G, R unless order == kJpegRGB), the return value the four
// luma bytes (what a gray output stores).  Pixels at or past the width are computed from plane padding and are the caller's to drop.
__device__ __forceinline__ uint32_t colour_quad(const uint8_t* __restrict__ base, const JpegGeom& g, int y, int x0, int order, uint8_t* px) {
    const int w = g.width, h = g.height;
    const int ys = g.blocks_w[0] * 8;
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(base + (size_t)y * ys + x0);     // inside the padded plane, 4-byte aligned
    int cb[4] = {128, 128, 128, 128}, cr[4] = {128, 128, 128, 128};
    if (g.ncomp == 3) {
        const int cs = g.blocks_w[1] * 8;
        const uint8_t* pb = base + g.plane_off[1];
        const uint8_t* pr = base + g.plane_off[2];
        if (g.hs == 1) {
            const uint32_t b4 = *reinterpret_cast<const uint32_t*>(pb + (size_t)y * cs + x0);
            const uint32_t r4 = *reinterpret_cast<const uint32_t*>(pr + (size_t)y * cs + x0);
#pragma unroll
            for (int i = 0; i < 4; ++i) { cb[i] = (b4 >> (8 * i)) & 255; cr[i] = (r4 >> (8 * i)) & 255; }
        } else {
            const int dw = (w + 1) >> 1, dh = g.vs == 2 ? (h + 1) >> 1 : h;
            const int r0 = g.vs == 2 ? y >> 1 : y;
            const int i0 = x0 >> 1;
            if (dw <= 2) {                                                               // libjpeg up-samples so narrow a plane by replication
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = min(i0 + (i >> 1), dw - 1);
                    cb[i] = pb[(size_t)r0 * cs + col];
                    cr[i] = pr[(size_t)r0 * cs + col];
                }
            } else {
                // column sums of the two rows that feed this output row (weights 3 : 1; one row with weight 4 when vs == 1), for the
                // columns i0 - 1 .. i0 + 2, clamped into the plane: a clamped column is never used, the edge rules below replace it
                const int r1 = g.vs == 2 ? ((y & 1) ? min(r0 + 1, dh - 1) : max(r0 - 1, 0)) : r0;
                int sb[4], sr[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int col = min(max(i0 - 1 + k, 0), dw - 1);
                    sb[k] = 3 * pb[(size_t)r0 * cs + col] + pb[(size_t)r1 * cs + col];
                    sr[k] = 3 * pr[(size_t)r0 * cs + col] + pr[(size_t)r1 * cs + col];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = i0 + (i >> 1), k = 1 + (i >> 1);
                    const bool edge = (i & 1) ? col >= dw - 1 : col == 0;
                    const int nb = (i & 1) ? k + 1 : k - 1;
                    if (g.vs == 2) {
                        // h2v2: (3 * this + neighbour + 8 | 7) >> 4 on the column sums; at the first / last column this * 4
                        const int rnd = (i & 1) ? 7 : 8;
                        cb[i] = ((edge ? 4 * sb[k] : 3 * sb[k] + sb[nb]) + rnd) >> 4;
                        cr[i] = ((edge ? 4 * sr[k] : 3 * sr[k] + sr[nb]) + rnd) >> 4;
                    } else {
                        // h2v1: (3 * this + neighbour + 1 | 2) >> 2 on the samples (sums are 4 * sample); the edge sample itself
                        const int rnd = (i & 1) ? 2 : 1;
                        cb[i] = edge ? sb[k] >> 2 : (3 * (sb[k] >> 2) + (sb[nb] >> 2) + rnd) >> 2;
                        cr[i] = edge ? sr[k] >> 2 : (3 * (sr[k] >> 2) + (sr[nb] >> 2) + rnd) >> 2;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = (y4 >> (8 * i)) & 255;
        int red = yy, green = yy, blue = yy;
        if (g.ncomp == 3) {
            const int u = cb[i] - 128, v = cr[i] - 128;
            red = clamp_u8(yy + ((91881 * v + 32768) >> 16));
            green = clamp_u8(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
            blue = clamp_u8(yy + ((116130 * u + 32768) >> 16));
        }
        px[3 * i] = (uint8_t)(order == kJpegRGB ? red : blue);
        px[3 * i + 1] = (uint8_t)green;
        px[3 * i + 2] = (uint8_t)(order == kJpegRGB ? blue : red);
    }
    return y4;
}

// One lane = four adjacent output pixels of one row.  `wide` (uniform): w is a multiple of 4 and dst is 4-byte aligned, so the lane
// stores 12 bytes (4 for gray) with one vector store; otherwise it stores bytes.
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, JpegGeom g, int n,
                                                          int order, int wide) {
    const int w = g.width, h = g.height, qw = (w + 3) >> 2;
    const size_t total = (size_t)n * h * qw;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int x0 = (int)(idx % qw) * 4;
    const size_t rest = idx / qw;
    const int y = (int)(rest % h);
    const size_t img = rest / h;
    uint8_t px[12];
    const uint32_t y4 = colour_quad(planes + img * ((size_t)g.blocks * 64), g, y, x0, order, px);
    const size_t p0 = (img * h + y) * (size_t)w + x0;
    if (order == kJpegGray) {
        if (wide) { *reinterpret_cast<uint32_t*>(dst + p0) = y4; return; }
        for (int i = 0; i < 4 && x0 + i < w; ++i) dst[p0 + i] = (uint8_t)(y4 >> (8 * i));
        return;
    }
    if (wide) {
        u32x3 o;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
        *reinterpret_cast<u32x3*>(dst + p0 * 3) = o;                                       // 12 bytes, 4-byte aligned
        return;
    }
    for (int i = 0; i < 4 && x0 + i < w; ++i)
        for (int k = 0; k < 3; ++k) dst[(p0 + i) * 3 + k] = px[3 * i + k];
}

// The colour stage with the EXIF orientation fused into its store.  A workgroup takes a kTile x kTile tile of SOURCE pixels; every lane
// does the plain kernel's per-lane work (colour_quad) and puts its pixels into LDS where the oriented picture has them, so that after
// the barrier LDS holds the byte image of an OUTPUT tile, row by row.  The tile is then written along output rows: every row of it is
// one contiguous run of 3 * width bytes (width bytes for gray) in dst, and lane (row, slot) owns the 4-byte ALIGNED word `slot` of that
// run -- one dword store where the word lies inside the run, byte stores for the ragged first and last word.  64 consecutive lanes
// cover two whole rows, and no lane ever stores a lone pixel at the stride of an output row, which is what swapping the indices of the
// plain kernel's store would do for the transposing tags.
//
// kTile = 32: 32 x 32 pixels are 256 x (4 pixels of one row), i.e. exactly one colour_quad per lane of the 256-lane group the plain kernel
// uses too, with nothing to loop over; the tile needs 3.2 KB of LDS, which never limits occupancy.  The tile also sets the smallest
// pictures at which the edge code can go wrong, i.e. the sizes the tests decode and their fixture stores.  A 64 x 64 tile (four quads per
// lane, 12.6 KB, runs of 192 bytes) was measured beside this one: 256 photos of 512 x 512 turn in 235 - 245 us instead of 277 - 287 us,
// the plain kernel's time.  That is 45 us beside a UNet of 53 ms for the same photos, and it quadruples the test pictures, so 32 stays
// (profiles/jpeg_orientation.md).  A row of the tile is 25 words apart (100 bytes): a multiple of 4, so that the alignment of a word
// inside its row is the same in LDS and in dst, and odd, so that the four pixels a lane scatters down a column for tags 5..8 fall into
// different banks.
//
// orient is 2..8 (uniform).  With a = the x coordinate and b = the y coordinate of a source pixel, mirrored inside the picture for
// tags {2, 3, 7, 8} and {3, 4, 6, 7} respectively, the output pixel is (row b, column a) for tags 2..4 and (row a, column b) for 5..8.
// Every address is a function of geometry and orientation alone.
constexpr int kTile = 32;
constexpr int kTileRowBytes = kTile * 3 + 4;
constexpr int kTileRowWords = kTileRowBytes / 4;
static_assert(kTile * kTile / 4 == 256 && kTileRowBytes % 4 == 0 && kTileRowWords % 2 == 1 && kTile * 3 / 4 + 1 <= kTile,
              "one quad per lane; word-aligned odd row pitch; a run touches at most kTile aligned words");

__global__ __launch_bounds__(256) void jpeg_colour_oriented_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, JpegGeom g,
                                                                   int order, int orient) {
    __shared__ uint32_t tile[kTile * kTileRowWords + 1];         // + 1: the funnel read below may look one word past the last run
    uint8_t* const tile8 = reinterpret_cast<uint8_t*>(tile);
    const int w = g.width, h = g.height;
    const unsigned tiles_x = (unsigned)(w + kTile - 1) / kTile, tiles_y = (unsigned)(h + kTile - 1) / kTile;
    const unsigned tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x, ty = rest % tiles_y;
    const size_t img = rest / tiles_y;
    const int sx0 = (int)tx * kTile, sy0 = (int)ty * kTile, tw = min(kTile, w - sx0), th = min(kTile, h - sy0);
    const bool transposed = orient >= 5;
    const bool mirror_x = orient == 2 || orient == 3 || orient == 7 || orient == 8;
    const bool mirror_y = orient == 3 || orient == 4 || orient == 6 || orient == 7;
    const int bpp = order == kJpegGray ? 1 : 3;

    const int ly = threadIdx.x / (kTile / 4), lx0 = (int)(threadIdx.x % (kTile / 4)) * 4;
    if (ly < th && lx0 < tw) {
        uint8_t px[12];
        const uint32_t y4 = colour_quad(planes + img * ((size_t)g.blocks * 64), g, sy0 + ly, sx0 + lx0, order, px);
        const int b = mirror_y ? th - 1 - ly : ly;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lx = lx0 + i;
            if (lx >= tw) break;
            const int a = mirror_x ? tw - 1 - lx : lx;
            uint8_t* p = tile8 + (transposed ? a : b) * kTileRowBytes + (transposed ? b : a) * bpp;
            if (order == kJpegGray) {
                p[0] = (uint8_t)(y4 >> (8 * i));
            } else {
                p[0] = px[3 * i]; p[1] = px[3 * i + 1]; p[2] = px[3 * i + 2];
            }
        }
    }
    __syncthreads();

    // the output tile: oh rows of `run` bytes, its first pixel at (oy0, ox0) of the (h2, w2) output picture
    const int oh = transposed ? tw : th, run = (transposed ? th : tw) * bpp;
    const int h2 = transposed ? w : h, w2 = transposed ? h : w;
    const int a0 = mirror_x ? w - sx0 - tw : sx0, b0 = mirror_y ? h - sy0 - th : sy0;
    const int oy0 = transposed ? a0 : b0, ox0 = transposed ? b0 : a0;
    for (int u = threadIdx.x; u < oh * kTile; u += 256) {
        const int r = u / kTile, slot = u % kTile;
        uint8_t* const first = dst + ((img * h2 + (size_t)(oy0 + r)) * (size_t)w2 + ox0) * bpp;     // the run is first[0 .. run)
        const int o = slot * 4 - (int)((uintptr_t)first & 3);                                        // first + o is 4-byte aligned
        if (o >= run) continue;
        const int at = r * kTileRowBytes + o;                                                      // the same four bytes in LDS
        if (o >= 0 && o + 4 <= run) {
            const uint64_t two = (uint64_t)tile[at >> 2] | (uint64_t)tile[(at >> 2) + 1] << 32;
            *reinterpret_cast<uint32_t*>(first + o) = (uint32_t)(two >> (8 * (at & 3)));
        } else {
            for (int j = 0; j < 4; ++j)
                if (o + j >= 0 && o + j < run) first[o + j] = tile8[at + j];
        }
    }
}

JpegGeom geom_of(const cvjpeg::Info& info) {
    const cvjpeg::Layout l = cvjpeg::layout_of(info);
    JpegGeom g;
    g.ncomp = l.ncomp; g.width = info.width; g.height = info.height;
    g.hs = l.ncomp == 3 ? info.luma_h : 1; g.vs = l.ncomp == 3 ? info.luma_v : 1;
    for (int c = 0; c < 3; ++c) {
        g.blocks_w[c] = l.blocks_w[c]; g.blocks_h[c] = l.blocks_h[c];
        g.block_off[c] = (unsigned)l.block_off[c];
        g.plane_off[c] = (unsigned)(l.block_off[c] * 64);
    }
    g.blocks = (unsigned)l.blocks;
    return g;
}

}  // namespace

size_t jpeg_planes_bytes(const cvjpeg::Info& info, int n) { return cvjpeg::layout_of(info).blocks * 64 * (size_t)(n > 0 ? n : 0); }

hipError_t jpeg_reconstruct_u8(const int16_t* coeffs, const uint16_t* qtables, int n, const cvjpeg::Info& info, int order, uint8_t* planes,
                               uint8_t* dst, hipStream_t s) {
    return jpeg_reconstruct_oriented_u8(coeffs, qtables, n, info, order, 0, planes, dst, s);
}

hipError_t jpeg_reconstruct_oriented_u8(const int16_t* coeffs, const uint16_t* qtables, int n, const cvjpeg::Info& info, int order,
                                        int orientation, uint8_t* planes, uint8_t* dst, hipStream_t s) {
    if (orientation < 0 || orientation > 8) return hipErrorInvalidValue;
    const JpegGeom g = geom_of(info);
    const size_t total_blocks = (size_t)g.blocks * n;
    const size_t groups = (total_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup;
    const size_t lanes = (size_t)n * g.height * ((g.width + 3) / 4);
    const size_t groups2 = (lanes + 255) / 256;
    const size_t tiles = (size_t)n * ((g.height + kTile - 1) / kTile) * ((g.width + kTile - 1) / kTile);
    if (groups == 0 || groups > 0x7fffffffu || groups2 > 0x7fffffffu || tiles > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(256), 0, s, coeffs, qtables, planes, g, total_blocks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (orientation >= 2) {                                    // tags 0 (absent) and 1 change nothing: the plain kernel below
        hipLaunchKernelGGL(jpeg_colour_oriented_kernel, dim3((unsigned)tiles), dim3(256), 0, s, planes, dst, g, order, orientation);
        return hipGetLastError();
    }
    const int wide = (g.width % 4 == 0) && ((uintptr_t)dst % 4 == 0);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)groups2), dim3(256), 0, s, planes, dst, g, n, order, wide);
    return hipGetLastError();
}

}  // namespace cv
