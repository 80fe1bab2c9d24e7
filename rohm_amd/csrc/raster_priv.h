// What the depth renderer (raster.hip) and the colour renderer (shade.hip) share: the camera, the per-triangle record, the
// coverage rule (tri_setup / tri_hit), the binning kernels and the per-tile merge loop.  The rule itself is stated in
// raster.hip and include/rohm_hip.h.  Contraction is off and every fused multiply-add is spelled out: both translation
// units must produce the same bits for the same triangle and pixel.
#pragma once
#include "common.h"
#include <limits.h>

#pragma clang fp contract(off)

namespace rohm {

constexpr int kTile = 64;
constexpr int kTilePix = kTile * kTile;
constexpr int kRasterWG = 256;
constexpr int kBinSpan = 4;           // a triangle touching more tiles than this goes to the large list
constexpr int kCoopArea = 64;         // clipped bounds above this many pixels: the whole workgroup shares the triangle
constexpr unsigned kNoHit = 0xffffffffu;

struct Camera {
    double fx, fy, cx, cy, znear, zfar;
    int W, H;
};

struct TriRec {
    double a[3], b[3], c[3];          // e_i(x, y) = a_i (x + 0.5) + b_i (y + 0.5) + c_i, multiplied by sign(det)
    double det;                       // |p0 . (p1 x p2)|
    int x0, y0, x1, y1;               // inclusive pixel bounds, clamped to the image
};

struct Xform {
    float m[12];                      // rows 0..2 of the 4 x 4 rigid transform
    int on;
};

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Edge functions, determinant and conservative pixel bounds of one camera-space triangle.  false: nothing to draw.
__device__ inline bool tri_setup(const double p[3][3], const Camera& cam, int cull, TriRec& r) {
    double n[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double* q = p[(i + 1) % 3];
        const double* s = p[(i + 2) % 3];
        n[i][0] = q[1] * s[2] - q[2] * s[1];
        n[i][1] = q[2] * s[0] - q[0] * s[2];
        n[i][2] = q[0] * s[1] - q[1] * s[0];
    }
    const double det = fma(p[0][0], n[0][0], fma(p[0][1], n[0][1], p[0][2] * n[0][2]));
    if (!(fabs(det) > 0.0) || !(fabs(det) < 1e300)) return false;      // degenerate, edge-on through the eye, or not finite
    if (cull && det > 0.0) return false;                                // clockwise as seen from the camera
    const double sg = det < 0.0 ? -1.0 : 1.0;
    const double zmax = fmax(p[0][2], fmax(p[1][2], p[2][2])), zmin = fmin(p[0][2], fmin(p[1][2], p[2][2]));
    if (!(zmax >= cam.znear) || !(zmin <= cam.zfar)) return false;
    // bounds of the triangle clipped against z = znear
    double ulo = 1e300, uhi = -1e300, vlo = 1e300, vhi = -1e300;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double* q = p[i];
        const double* s = p[(i + 1) % 3];
        if (q[2] >= cam.znear) {
            const double u = q[0] / q[2] * cam.fx + cam.cx, v = q[1] / q[2] * cam.fy + cam.cy;
            ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
        }
        if ((q[2] >= cam.znear) != (s[2] >= cam.znear)) {
            const double t = (cam.znear - q[2]) / (s[2] - q[2]);
            const double px = q[0] + t * (s[0] - q[0]), py = q[1] + t * (s[1] - q[1]);
            const double u = px / cam.znear * cam.fx + cam.cx, v = py / cam.znear * cam.fy + cam.cy;
            ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
        }
    }
    if (!(ulo <= uhi) || !(vlo <= vhi)) return false;
    // a sample x + 0.5 inside [ulo, uhi] has x in [floor(ulo) - 1, floor(uhi) + 1]: at least half a pixel of slack
    const double W2 = (double)cam.W + 2.0, H2 = (double)cam.H + 2.0;
    int x0 = (int)floor(clampd(ulo, -2.0, W2)) - 1, x1 = (int)floor(clampd(uhi, -2.0, W2)) + 1;
    int y0 = (int)floor(clampd(vlo, -2.0, H2)) - 1, y1 = (int)floor(clampd(vhi, -2.0, H2)) + 1;
    if (x1 < 0 || y1 < 0 || x0 > cam.W - 1 || y0 > cam.H - 1) return false;
    r.x0 = x0 < 0 ? 0 : x0, r.y0 = y0 < 0 ? 0 : y0;
    r.x1 = x1 > cam.W - 1 ? cam.W - 1 : x1, r.y1 = y1 > cam.H - 1 ? cam.H - 1 : y1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = sg * n[i][0] / cam.fx, b = sg * n[i][1] / cam.fy;
        r.a[i] = a, r.b[i] = b;
        r.c[i] = sg * n[i][2] - a * cam.cx - b * cam.cy;
    }
    r.det = fabs(det);
    return true;
}

// The coverage rule at pixel (x, y), which must lie inside the image.  On a hit *bits receives the fp32 depth's pattern.
__device__ __forceinline__ bool tri_hit(const TriRec& r, int x, int y, double znear, double zfar, unsigned* bits) {
    const double u = (double)x + 0.5, v = (double)y + 0.5;
    const double e0 = fma(r.a[0], u, fma(r.b[0], v, r.c[0]));
    const double e1 = fma(r.a[1], u, fma(r.b[1], v, r.c[1]));
    const double e2 = fma(r.a[2], u, fma(r.b[2], v, r.c[2]));
    if (!(e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0)) return false;
    const double s = (e0 + e1) + e2;
    if (!(s > 0.0)) return false;
    const double z = r.det / s;
    if (!(z >= znear && z <= zfar)) return false;
    const float zf = (float)z;
    if (!(zf > 0.f) || !(zf < 3.0e38f)) return false;      // keep the pattern a positive finite float below kNoHit
    *bits = __float_as_uint(zf);
    return true;
}

// Vertices of face f of mesh `mesh` in camera space (fp64), false if an index is out of range.
__device__ __forceinline__ bool load_tri(const float* __restrict__ verts, const int* __restrict__ faces, int V, int mesh, int f,
                                         const Xform& xf, double p[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int vi = faces[(size_t)f * 3 + k];
        if (vi < 0 || vi >= V) return false;
        const float* q = verts + ((size_t)mesh * V + vi) * 3;
        const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
        if (xf.on) {
#pragma unroll
            for (int row = 0; row < 3; ++row)
                p[k][row] = fma((double)xf.m[row * 4 + 0], x, fma((double)xf.m[row * 4 + 1], y,
                                fma((double)xf.m[row * 4 + 2], z, (double)xf.m[row * 4 + 3])));
        } else {
            p[k][0] = x, p[k][1] = y, p[k][2] = z;
        }
    }
    return true;
}

// ---- rendering ------------------------------------------------------------------------------------------------------
struct RenderWs {
    TriRec* rec;              // [n_mesh * F]
    unsigned* count;          // [n_mesh * n_tiles + 1]: per-tile counts, then exclusive offsets (scan in place)
    unsigned* cursor;         // [n_mesh * n_tiles]
    unsigned* big_count;      // [n_mesh]
    int* big;                 // [n_mesh * F]
    int* refs;                // [kBinSpan * n_mesh * F]
};

static __global__ __launch_bounds__(kRasterWG) void raster_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 int V, int F, int n_mesh, Xform xf, Camera cam, int cull,
                                                                 int tiles_x, int n_tiles, RenderWs ws) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i >= (long long)n_mesh * F) return;
    const int mesh = (int)(i / F), f = (int)(i - (long long)mesh * F);
    TriRec r;
    double p[3][3];
    r.x0 = 0, r.x1 = -1, r.y0 = 0, r.y1 = -1;                 // marks "nothing to draw" for the fill pass
    const bool ok = load_tri(verts, faces, V, mesh, f, xf, p) && tri_setup(p, cam, cull, r);
    ws.rec[i] = r;
    if (!ok) return;
    const int tx0 = r.x0 / kTile, tx1 = r.x1 / kTile, ty0 = r.y0 / kTile, ty1 = r.y1 / kTile;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > kBinSpan) {
        const unsigned k = atomicAdd(&ws.big_count[mesh], 1u);
        ws.big[(size_t)mesh * F + k] = f;
        return;
    }
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&ws.count[(size_t)mesh * n_tiles + ty * tiles_x + tx], 1u);
}

// exclusive scan of count[0 .. n) in place, count[n] = total; one workgroup
static __global__ __launch_bounds__(1024) void raster_scan_kernel(unsigned* __restrict__ count, unsigned* __restrict__ cursor, long long n) {
    __shared__ unsigned sh[1024];
    __shared__ unsigned carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + tid;
        const unsigned v = i < n ? count[i] : 0u;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const unsigned t = tid >= o ? sh[tid - o] : 0u;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        const unsigned excl = carry + sh[tid] - v;
        if (i < n) {
            count[i] = excl;
            cursor[i] = excl;
        }
        __syncthreads();
        if (tid == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (tid == 0) count[n] = carry;
}

static __global__ __launch_bounds__(kRasterWG) void raster_fill_kernel(int F, int n_mesh, int tiles_x, int n_tiles, RenderWs ws) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i >= (long long)n_mesh * F) return;
    const int mesh = (int)(i / F), f = (int)(i - (long long)mesh * F);
    const TriRec& r = ws.rec[i];
    if (r.x1 < r.x0) return;
    const int tx0 = r.x0 / kTile, tx1 = r.x1 / kTile, ty0 = r.y0 / kTile, ty1 = r.y1 / kTile;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > kBinSpan) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const unsigned k = atomicAdd(&ws.cursor[(size_t)mesh * n_tiles + ty * tiles_x + tx], 1u);
            ws.refs[k] = f;
        }
}

// One tile's triangles merged into its LDS z-buffer `zbuf` [kTilePix]; every thread of the workgroup calls it.  Key is the
// 32-bit depth pattern (depth only) or (depth pattern << 32) | face (colour: among equal depths the smallest face index
// wins); both merge with an unsigned atomic min, so the result does not depend on the order the bins were filled in.
__device__ __forceinline__ void tile_merge(unsigned* cell, unsigned bits, int) { atomicMin(cell, bits); }
__device__ __forceinline__ void tile_merge(unsigned long long* cell, unsigned bits, int f) {
    atomicMin(cell, ((unsigned long long)bits << 32) | (unsigned)f);
}

template <typename Key>
__device__ __forceinline__ void rasterise_tile(Key* zbuf, int* queue, int* n_queue, int F, const Camera& cam, int tiles_x,
                                               int n_tiles, const RenderWs& ws) {
    const int tid = threadIdx.x;
    const int mesh = blockIdx.x / n_tiles, tile = blockIdx.x - mesh * n_tiles;
    const int ox = (tile % tiles_x) * kTile, oy = (tile / tiles_x) * kTile;
    const int tx1 = min(ox + kTile, cam.W) - 1, ty1 = min(oy + kTile, cam.H) - 1;
    for (int k = tid; k < kTilePix; k += kRasterWG) zbuf[k] = ~(Key)0;
    if (tid == 0) *n_queue = 0;
    const unsigned off = ws.count[blockIdx.x], n_bin = ws.count[blockIdx.x + 1] - off, n_big = ws.big_count[mesh];
    const TriRec* rec = ws.rec + (size_t)mesh * F;
    const int* big = ws.big + (size_t)mesh * F;
    __syncthreads();
    for (unsigned base = 0; base < n_bin + n_big; base += kRasterWG) {
        const unsigned k = base + tid;
        if (k < n_bin + n_big) {
            const int f = k < n_bin ? ws.refs[off + k] : big[k - n_bin];
            const TriRec& r = rec[f];
            const int x0 = max(r.x0, ox), x1 = min(r.x1, tx1), y0 = max(r.y0, oy), y1 = min(r.y1, ty1);
            if (x0 <= x1 && y0 <= y1) {
                if ((x1 - x0 + 1) * (y1 - y0 + 1) > kCoopArea) {
                    queue[atomicAdd(n_queue, 1)] = f;
                } else {
                    for (int y = y0; y <= y1; ++y)
                        for (int x = x0; x <= x1; ++x) {
                            unsigned bits;
                            if (tri_hit(r, x, y, cam.znear, cam.zfar, &bits)) tile_merge(&zbuf[(y - oy) * kTile + (x - ox)], bits, f);
                        }
                }
            }
        }
        __syncthreads();
        const int nq = *n_queue;
        for (int q = 0; q < nq; ++q) {
            const int f = queue[q];
            const TriRec& r = rec[f];
            const int x0 = max(r.x0, ox), x1 = min(r.x1, tx1), y0 = max(r.y0, oy), y1 = min(r.y1, ty1);
            const int w = x1 - x0 + 1, npx = w * (y1 - y0 + 1);
            for (int i = tid; i < npx; i += kRasterWG) {
                const int y = y0 + i / w, x = x0 + i % w;
                unsigned bits;
                if (tri_hit(r, x, y, cam.znear, cam.zfar, &bits)) tile_merge(&zbuf[(y - oy) * kTile + (x - ox)], bits, f);
            }
        }
        __syncthreads();
        if (tid == 0) *n_queue = 0;
        __syncthreads();
    }
}

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

static RenderWs carve(void* ws, int n_mesh, long long nt, long long n_mt, size_t* total) {
    RenderWs w;
    size_t o = 0;
    char* base = (char*)ws;
    w.rec = (TriRec*)(base + o), o += align256(sizeof(TriRec) * (size_t)nt);
    w.count = (unsigned*)(base + o), o += align256(4 * (size_t)(n_mt + 1));
    w.cursor = (unsigned*)(base + o), o += align256(4 * (size_t)n_mt);
    w.big_count = (unsigned*)(base + o), o += align256(4 * (size_t)n_mesh);
    w.big = (int*)(base + o), o += align256(4 * (size_t)nt);
    w.refs = (int*)(base + o), o += align256(4 * (size_t)kBinSpan * (size_t)nt);
    *total = o;
    return w;
}

static int check_camera(const char* who, double fx, double fy, int W, int H, double znear, double zfar) {
    ROHM_ARG_CHECK(W > 0 && H > 0 && W <= 16384 && H <= 16384, "%s: image size %d x %d out of range (1 .. 16384)", who, W, H);
    ROHM_ARG_CHECK(fx > 0 && fy > 0, "%s: focal lengths must be positive", who);
    ROHM_ARG_CHECK(znear > 0 && zfar > znear, "%s: need 0 < znear < zfar (got %g, %g)", who, znear, zfar);
    return ROHM_OK;
}

static Xform make_xform(const float* transform) {
    Xform xf;
    xf.on = transform != nullptr;
    for (int k = 0; k < 12; ++k) xf.m[k] = transform ? transform[k] : 0.f;
    return xf;
}

// Setup, count, scan and fill: after it `w` holds every triangle's record, the per-(mesh, tile) bins and the large lists.
static int bin_triangles(const float* verts, const int* faces, int n_mesh, int V, int F, const Xform& xf, const Camera& cam, int cull,
                         int tiles_x, int n_tiles, const RenderWs& w, hipStream_t s) {
    const long long nt = (long long)n_mesh * F, n_mt = (long long)n_mesh * n_tiles;
    // counts, cursors and the large-list counters are contiguous
    ROHM_HIP_CHECK(hipMemsetAsync(w.count, 0, (size_t)((char*)w.big - (char*)w.count), s));
    const unsigned g = (unsigned)((nt + kRasterWG - 1) / kRasterWG);
    hipLaunchKernelGGL(raster_setup_kernel, dim3(g), dim3(kRasterWG), 0, s, verts, faces, V, F, n_mesh, xf, cam, cull, tiles_x, n_tiles,
                       w);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, w.cursor, n_mt);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_fill_kernel, dim3(g), dim3(kRasterWG), 0, s, F, n_mesh, tiles_x, n_tiles, w);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

}  // namespace rohm
