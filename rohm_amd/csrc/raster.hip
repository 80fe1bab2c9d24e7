// Depth rendering and PROX joint-occlusion masks on the device: utils/get_occlusion_mask.py:63-143.
//
// The script renders the static scene and every frame's SMPL-X body with pyrender (an IntrinsicsCamera under the pose
// diag(1, -1, -1, 1)), projects 25 joints with cv2.projectPoints and calls a joint occluded where the body's depth lies
// more than 0.1 m behind the scene's.  Here that is three pieces: a depth renderer, a depth probe at listed pixels and
// the projection + decision.
//
// Coverage rule (one rule for the renderer, the probe and tests/raster_ref.py):
//   * The camera is a pinhole in OpenCV axes -- x right, y down, z forward -- which is what pyrender's IntrinsicsCamera
//     under the script's diag(1, -1, -1, 1) pose amounts to.  Pixel (x, y) samples the ray through u = x + 0.5,
//     v = y + 0.5, i.e. the direction d = ((u - cx) / fx, (v - cy) / fy, 1).
//   * The depth of a pixel is the smallest camera-space z at which that ray meets any triangle, znear <= z <= zfar
//     (pyrender's defaults are 0.05 and 100); 0 where nothing is hit.
//   * Meshes are two-sided.  With the cull flag, triangles whose vertices run clockwise as seen from the camera are
//     dropped, as OpenGL's default back-face culling under pyrender does; scene scans are open surfaces, so the two
//     differ wherever a surface is seen from behind.
//
// No clipper: a triangle (p0, p1, p2) is tested through its homogeneous edge functions e_i(d) = (p_j x p_k) . d.  The ray
// meets the triangle in front of the camera iff all e_i have the sign of det = p0 . (p1 x p2) and their sum is non-zero;
// then z = det / (e_0 + e_1 + e_2).  This holds unchanged for triangles that cross z = 0 or lie behind the camera (PROX
// scenes surround it).  The e_i are affine in the pixel coordinates; coefficients and evaluation are fp64 (at u ~ 1920
// fp32 edge functions carry ~1e-3 px of error), the stored depth is fp32.  Contraction is off and every fused
// multiply-add is spelled out, so the renderer and the probe -- which share tri_setup and tri_hit -- produce the same
// bits for the same triangle and pixel.
//
// Rendering: setup + count, a single-workgroup scan over the (mesh, tile) counters, fill, then one workgroup per
// 64 x 64 tile with its z-buffer in LDS (16 KB).  Bounds come from the triangle clipped against z = znear (bounds only:
// the test itself never clips), so a triangle that crosses the near plane reaches every tile its clipped bounds touch.
// A triangle spanning at most 4 tiles is binned (<= 4 references each, which bounds the scratch); a larger one goes to
// its mesh's list of large triangles, which every tile of that mesh walks.  Depths are merged with an unsigned min on
// the bit pattern of the positive float: order-independent, hence bitwise reproducible whatever order the atomics
// filled the bins in.  The camera, the per-triangle record, tri_setup / tri_hit, the binning kernels and the per-tile merge
// loop live in raster_priv.h, which the colour renderer (shade.hip) shares.
#include "raster_priv.h"

#pragma clang fp contract(off)

namespace rohm {

// ---- rendering ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRasterWG) void raster_tile_kernel(float* __restrict__ depth, int F, Camera cam, int tiles_x, int n_tiles,
                                                                RenderWs ws) {
    __shared__ unsigned zbuf[kTilePix];
    __shared__ int queue[kRasterWG];
    __shared__ int n_queue;
    rasterise_tile(zbuf, queue, &n_queue, F, cam, tiles_x, n_tiles, ws);
    const int tid = threadIdx.x;
    const int mesh = blockIdx.x / n_tiles, tile = blockIdx.x - mesh * n_tiles;
    const int ox = (tile % tiles_x) * kTile, oy = (tile / tiles_x) * kTile;
    float* img = depth + (size_t)mesh * cam.W * cam.H;
    for (int k = tid; k < kTilePix; k += kRasterWG) {
        const int x = ox + (k % kTile), y = oy + (k / kTile);
        if (x < cam.W && y < cam.H) {
            const unsigned b = zbuf[k];
            img[(size_t)y * cam.W + x] = b == kNoHit ? 0.f : __uint_as_float(b);
        }
    }
}

// ---- probe ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRasterWG) void raster_fill_u32_kernel(unsigned* __restrict__ out, long long n, unsigned v) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i < n) out[i] = v;
}

__global__ __launch_bounds__(kRasterWG) void raster_probe_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 int V, int F, int n_mesh, Xform xf, Camera cam, int cull,
                                                                 const int* __restrict__ pix, int P, unsigned* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i >= (long long)n_mesh * F) return;
    const int mesh = (int)(i / F), f = (int)(i - (long long)mesh * F);
    TriRec r;
    double p[3][3];
    if (!load_tri(verts, faces, V, mesh, f, xf, p) || !tri_setup(p, cam, cull, r)) return;
    const int* px = pix + (size_t)mesh * P * 2;
    unsigned* o = out + (size_t)mesh * P;
    for (int k = 0; k < P; ++k) {
        const int x = px[2 * k], y = px[2 * k + 1];
        if (x < r.x0 || x > r.x1 || y < r.y0 || y > r.y1) continue;       // the bounds lie inside the image
        unsigned bits;
        if (tri_hit(r, x, y, cam.znear, cam.zfar, &bits)) atomicMin(&o[k], bits);
    }
}

__global__ __launch_bounds__(kRasterWG) void raster_probe_finish_kernel(unsigned* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i < n && out[i] == kNoHit) out[i] = 0u;                            // 0.0f
}

// ---- projection and decision ----------------------------------------------------------------------------------------
struct Lens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// cv2.projectPoints with zero rvec / tvec and five coefficients (k1, k2, p1, p2, k3), in double as OpenCV computes it:
// x' = X / Z, y' = Y / Z (Z == 0 divides by 1), r2 = x'^2 + y'^2,
// x" = x' (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x' y' + p2 (r2 + 2 x'^2), y" likewise, u = fx x" + cx, v = fy y" + cy;
// then numpy's astype(int): truncation toward zero.  A value that does not fit lands outside every image.
__device__ __forceinline__ int trunc_pixel(double u) {
    if (!(fabs(u) < 2.0e9)) return INT_MIN;
    return (int)u;
}

__device__ __forceinline__ void project_joint(const float* __restrict__ j, const Lens& L, int* x, int* y) {
    const double X = (double)j[0], Y = (double)j[1], Z = (double)j[2];
    const double iz = Z != 0.0 ? 1.0 / Z : 1.0;
    const double xp = X * iz, yp = Y * iz;
    const double r2 = xp * xp + yp * yp, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2.0 * xp * yp, a2 = r2 + 2.0 * xp * xp, a3 = r2 + 2.0 * yp * yp;
    const double cdist = 1.0 + L.k1 * r2 + L.k2 * r4 + L.k3 * r6;
    const double xd = xp * cdist + L.p1 * a1 + L.p2 * a2, yd = yp * cdist + L.p1 * a3 + L.p2 * a1;
    *x = trunc_pixel(xd * L.fx + L.cx);
    *y = trunc_pixel(yd * L.fy + L.cy);
}

__global__ __launch_bounds__(kRasterWG) void project_pixels_kernel(const float* __restrict__ joints, Lens L, long long n,
                                                                   int* __restrict__ pix) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i >= n) return;
    int x, y;
    project_joint(joints + i * 3, L, &x, &y);
    pix[2 * i] = x, pix[2 * i + 1] = y;
}

// get_occlusion_mask.py:138-143 on float32 depth images: occluded iff inside the image, scene != 0 and body - scene > thr
__global__ __launch_bounds__(kRasterWG) void occlusion_decide_kernel(const float* __restrict__ joints, Lens L,
                                                                     const float* __restrict__ scene, int W, int H,
                                                                     const float* __restrict__ body, float thr, long long n,
                                                                     float* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    if (i >= n) return;
    int x, y;
    project_joint(joints + i * 3, L, &x, &y);
    float m = 1.f;
    if (x >= 0 && x < W && y >= 0 && y < H) {
        const float s = scene[(size_t)y * W + x];
        if (body[i] - s > thr && s != 0.f) m = 0.f;
    }
    mask[i] = m;
}

static int make_lens(const char* who, const double* camera_mtx, const double* dist, Lens* L) {
    ROHM_ARG_CHECK(camera_mtx && dist, "%s: camera matrix and distortion coefficients are required", who);
    L->fx = camera_mtx[0], L->fy = camera_mtx[4], L->cx = camera_mtx[2], L->cy = camera_mtx[5];
    L->k1 = dist[0], L->k2 = dist[1], L->p1 = dist[2], L->p2 = dist[3], L->k3 = dist[4];
    return ROHM_OK;
}

}  // namespace rohm

using namespace rohm;

extern "C" size_t rohm_depth_workspace_bytes(int n_mesh, int F, int W, int H) {
    if (n_mesh <= 0 || F <= 0 || W <= 0 || H <= 0) return 0;
    const long long tiles = (long long)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    size_t total = 0;
    carve(nullptr, n_mesh, (long long)n_mesh * F, (long long)n_mesh * tiles, &total);
    return total;
}

extern "C" int rohm_depth_render(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform,
                                 double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar,
                                 int cull_backfaces, float* depth, void* ws, size_t ws_bytes, rohm_stream_t stream) {
    ROHM_ARG_CHECK(verts && faces && depth && ws, "depth_render: null argument");
    ROHM_ARG_CHECK(n_mesh > 0 && V > 0 && F > 0, "depth_render: need n_mesh, V, F > 0 (got %d, %d, %d)", n_mesh, V, F);
    if (int rc = check_camera("depth_render", fx, fy, W, H, znear, zfar)) return rc;
    const long long nt = (long long)n_mesh * F;
    const int tiles_x = (W + kTile - 1) / kTile, n_tiles = tiles_x * ((H + kTile - 1) / kTile);
    const long long n_mt = (long long)n_mesh * n_tiles;
    ROHM_ARG_CHECK(nt * kBinSpan < (1ll << 31) && n_mt < (1ll << 31) && (long long)n_mesh * V < (1ll << 31),
                   "depth_render: batch too large (%d meshes x %d faces): split the call", n_mesh, F);
    size_t need = 0;
    RenderWs w = carve(ws, n_mesh, nt, n_mt, &need);
    if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        set_error("depth_render: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", need, ws_bytes);
        return ROHM_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Camera cam{fx, fy, cx, cy, znear, zfar, W, H};
    const Xform xf = make_xform(transform);
    prof::Scope ps("depth_render", 60.0 * nt, (double)sizeof(TriRec) * 2 * nt + 4.0 * n_mesh * W * H, s);
    if (int rc = bin_triangles(verts, faces, n_mesh, V, F, xf, cam, cull_backfaces, tiles_x, n_tiles, w, s)) return rc;
    hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)n_mt), dim3(kRasterWG), 0, s, depth, F, cam, tiles_x, n_tiles, w);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_depth_probe(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform,
                                double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar,
                                int cull_backfaces, const int* pixels, int P, float* depth, rohm_stream_t stream) {
    ROHM_ARG_CHECK(verts && faces && pixels && depth, "depth_probe: null argument");
    ROHM_ARG_CHECK(n_mesh > 0 && V > 0 && F > 0 && P > 0, "depth_probe: need n_mesh, V, F, P > 0 (got %d, %d, %d, %d)", n_mesh, V,
                   F, P);
    if (int rc = check_camera("depth_probe", fx, fy, W, H, znear, zfar)) return rc;
    const long long nt = (long long)n_mesh * F, np = (long long)n_mesh * P;
    ROHM_ARG_CHECK(nt < (1ll << 39) && (nt + kRasterWG - 1) / kRasterWG < (1ll << 31), "depth_probe: batch too large: split the call");
    hipStream_t s = (hipStream_t)stream;
    const Camera cam{fx, fy, cx, cy, znear, zfar, W, H};
    const Xform xf = make_xform(transform);
    prof::Scope ps("depth_probe", 60.0 * nt, 48.0 * nt + 12.0 * np, s);
    unsigned* out = (unsigned*)depth;
    const unsigned gp = (unsigned)((np + kRasterWG - 1) / kRasterWG);
    hipLaunchKernelGGL(raster_fill_u32_kernel, dim3(gp), dim3(kRasterWG), 0, s, out, np, kNoHit);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_probe_kernel, dim3((unsigned)((nt + kRasterWG - 1) / kRasterWG)), dim3(kRasterWG), 0, s, verts, faces, V,
                       F, n_mesh, xf, cam, cull_backfaces, pixels, P, out);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_probe_finish_kernel, dim3(gp), dim3(kRasterWG), 0, s, out, np);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_project_pixels(const float* joints, const double* camera_mtx, const double* dist, int N, int J, int* pixels,
                                   rohm_stream_t stream) {
    ROHM_ARG_CHECK(joints && pixels && N > 0 && J > 0, "project_pixels: null or empty argument");
    Lens L;
    if (int rc = make_lens("project_pixels", camera_mtx, dist, &L)) return rc;
    const long long n = (long long)N * J;
    hipLaunchKernelGGL(project_pixels_kernel, dim3((unsigned)((n + kRasterWG - 1) / kRasterWG)), dim3(kRasterWG), 0, (hipStream_t)stream,
                       joints, L, n, pixels);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_joint_occlusion_mask(const float* joints, const double* camera_mtx, const double* dist,
                                         const float* scene_depth, int W, int H, const float* body_depth, float thr, int N, int J,
                                         float* mask, rohm_stream_t stream) {
    ROHM_ARG_CHECK(joints && scene_depth && body_depth && mask && N > 0 && J > 0, "joint_occlusion_mask: null or empty argument");
    ROHM_ARG_CHECK(W > 0 && H > 0, "joint_occlusion_mask: image size %d x %d", W, H);
    Lens L;
    if (int rc = make_lens("joint_occlusion_mask", camera_mtx, dist, &L)) return rc;
    const long long n = (long long)N * J;
    hipLaunchKernelGGL(occlusion_decide_kernel, dim3((unsigned)((n + kRasterWG - 1) / kRasterWG)), dim3(kRasterWG), 0,
                       (hipStream_t)stream, joints, L, scene_depth, W, H, body_depth, thr, n, mask);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
