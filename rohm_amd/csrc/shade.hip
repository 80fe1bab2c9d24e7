// Evaluation pictures on the device: what eval_amass_full.py:277-395, eval_prox_egobody.py:373-451 and utils/render_util.py
// do with pyrender, trimesh, an OpenGL context and PIL.  Smooth vertex normals, a shaded colour render on top of the depth
// renderer's coverage rule (raster_priv.h), the skeleton's spheres and cylinders as one batched mesh, and the scripts' image
// arithmetic on uint8 images.
//
// Shading rule (one rule for the kernel and tests/shade_ref.py; include/rohm_hip.h states it in full):
//   * coverage and depth are the depth renderer's, bit for bit; the winner of a pixel is the smallest fp32 depth pattern and,
//     among equal patterns, the smallest face index: a 64-bit key (depth bits << 32) | face per pixel in the tile's LDS
//     z-buffer (32 KB), merged with an unsigned 64-bit atomic min -- order-independent, hence bitwise reproducible;
//   * resolve, once per covered pixel: weights l_i = e_i / (e_0 + e_1 + e_2) from the winner's fp64 edge functions (the
//     perspective-correct barycentrics of the hit point), n = normalise(sum l_i n_i) in camera space (or the face normal),
//     turned toward the eye unless back faces are culled, one directional light along the viewing axis:
//     lambert = max(0, -n_z), out_k = floor(255 min(1, c_k (ambient + diffuse lambert)) + 0.5), out_a = floor(255 a + 0.5).
//     Shading arithmetic is fp32.  No specular term, no sRGB curve, no blending behind a translucent surface.
#include "raster_priv.h"

#pragma clang fp contract(off)

namespace rohm {

constexpr int kShadeWG = 256;

// ---- vertex normals -------------------------------------------------------------------------------------------------
// Gather form: thread (mesh, vertex) sums the un-normalised (p1 - p0) x (p2 - p0) of its incident faces in list order
// (area weighting) and normalises; no atomics, so the bits do not depend on scheduling.
__global__ __launch_bounds__(kShadeWG) void vertex_normals_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  const int* __restrict__ offsets, const int* __restrict__ face_ids,
                                                                  int n_mesh, int V, int F, float* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= (long long)n_mesh * V) return;
    const int mesh = (int)(i / V), v = (int)(i - (long long)mesh * V);
    const float* base = verts + (size_t)mesh * V * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int k0 = offsets[v], k1 = offsets[v + 1];
    if (k0 < 0) k0 = 0;
    if (k1 > 3 * F) k1 = 3 * F;
    for (int k = k0; k < k1; ++k) {
        const int f = face_ids[k];
        if (f < 0 || f >= F) continue;
        const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
        const float* p0 = base + (size_t)i0 * 3;
        const float* p1 = base + (size_t)i1 * 3;
        const float* p2 = base + (size_t)i2 * 3;
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        sx += ay * bz - az * by;
        sy += az * bx - ax * bz;
        sz += ax * by - ay * bx;
    }
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    float* o = normals + i * 3;
    if (len > 0.f && len < 3.0e38f) {
        o[0] = sx / len, o[1] = sy / len, o[2] = sz / len;
    } else {
        o[0] = 0.f, o[1] = 0.f, o[2] = 0.f;
    }
}

// ---- colour render --------------------------------------------------------------------------------------------------
struct ShadeArgs {
    const float* verts;
    const int* faces;
    const float* normals;             // [n_mesh, V, 3] or null: flat shading
    const unsigned char* colors;      // [n_mesh or 1, V, 4]
    int V, colors_per_mesh, cull;
    float ambient, diffuse;
    unsigned char* rgba;              // [n_mesh, H, W, 4]
    float* depth;                     // [n_mesh, H, W] or null
    int* face_id;                     // [n_mesh, H, W] or null
};

__device__ __forceinline__ unsigned char to_level(float v) {
    const float q = floorf(255.f * v + 0.5f);
    return (unsigned char)(q < 0.f ? 0.f : (q > 255.f ? 255.f : q));
}

__device__ void resolve_pixel(const ShadeArgs& a, const Xform& xf, const Camera& cam, const TriRec& r, int mesh, int f, int x, int y,
                              unsigned char out[4]) {
    const double u = (double)x + 0.5, v = (double)y + 0.5;
    const double e0 = fma(r.a[0], u, fma(r.b[0], v, r.c[0]));
    const double e1 = fma(r.a[1], u, fma(r.b[1], v, r.c[1]));
    const double e2 = fma(r.a[2], u, fma(r.b[2], v, r.c[2]));
    const double s = (e0 + e1) + e2;                  // > 0: the pixel was hit
    const float l[3] = {(float)(e0 / s), (float)(e1 / s), (float)(e2 / s)};
    int vi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vi[k] = a.faces[(size_t)f * 3 + k];      // in range: the face was set up
    float n[3] = {0.f, 0.f, 0.f};
    if (a.normals) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* q = a.normals + ((size_t)mesh * a.V + vi[k]) * 3;
            float c[3] = {q[0], q[1], q[2]};
            if (xf.on) {
#pragma unroll
                for (int row = 0; row < 3; ++row)
                    c[row] = xf.m[row * 4 + 0] * q[0] + xf.m[row * 4 + 1] * q[1] + xf.m[row * 4 + 2] * q[2];
            }
            n[0] += l[k] * c[0], n[1] += l[k] * c[1], n[2] += l[k] * c[2];
        }
    } else {
        double p[3][3];
        load_tri(a.verts, a.faces, a.V, mesh, f, xf, p);
        const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
        const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
        n[0] = (float)(ay * bz - az * by), n[1] = (float)(az * bx - ax * bz), n[2] = (float)(ax * by - ay * bx);
    }
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (len > 0.f && len < 3.0e38f) {
        n[0] /= len, n[1] /= len, n[2] /= len;
    } else {
        n[0] = n[1] = n[2] = 0.f;
    }
    const float dx = (float)((u - cam.cx) / cam.fx), dy = (float)((v - cam.cy) / cam.fy);
    if (!a.cull && n[0] * dx + n[1] * dy + n[2] > 0.f) n[2] = -n[2];      // only n_z enters the light term
    const float shade = a.ambient + a.diffuse * fmaxf(0.f, -n[2]);
    const unsigned char* cb = a.colors + (size_t)(a.colors_per_mesh ? mesh : 0) * a.V * 4;
    const unsigned char* c0 = cb + (size_t)vi[0] * 4;
    const unsigned char* c1 = cb + (size_t)vi[1] * 4;
    const unsigned char* c2 = cb + (size_t)vi[2] * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float c = (l[0] * (float)c0[k] + l[1] * (float)c1[k] + l[2] * (float)c2[k]) / 255.f;
        out[k] = to_level(k < 3 ? fminf(1.f, c * shade) : c);
    }
}

__global__ __launch_bounds__(kRasterWG) void shade_tile_kernel(ShadeArgs a, Xform xf, int F, Camera cam, int tiles_x, int n_tiles,
                                                               RenderWs ws) {
    __shared__ unsigned long long zbuf[kTilePix];
    __shared__ int queue[kRasterWG];
    __shared__ int n_queue;
    rasterise_tile(zbuf, queue, &n_queue, F, cam, tiles_x, n_tiles, ws);
    const int tid = threadIdx.x;
    const int mesh = blockIdx.x / n_tiles, tile = blockIdx.x - mesh * n_tiles;
    const int ox = (tile % tiles_x) * kTile, oy = (tile / tiles_x) * kTile;
    const TriRec* rec = ws.rec + (size_t)mesh * F;
    const size_t img = (size_t)mesh * cam.W * cam.H;
    for (int k = tid; k < kTilePix; k += kRasterWG) {
        const int x = ox + (k % kTile), y = oy + (k / kTile);
        if (x >= cam.W || y >= cam.H) continue;
        const unsigned long long key = zbuf[k];
        const size_t at = img + (size_t)y * cam.W + x;
        uchar4 px = make_uchar4(0, 0, 0, 0);
        float z = 0.f;
        int f = -1;
        if (key != ~0ull) {
            f = (int)(unsigned)(key & 0xffffffffull);
            z = __uint_as_float((unsigned)(key >> 32));
            unsigned char c[4];
            resolve_pixel(a, xf, cam, rec[f], mesh, f, x, y, c);
            px = make_uchar4(c[0], c[1], c[2], c[3]);
        }
        ((uchar4*)a.rgba)[at] = px;
        if (a.depth) a.depth[at] = z;
        if (a.face_id) a.face_id[at] = f;
    }
}

// ---- skeleton -------------------------------------------------------------------------------------------------------
// create_pyrender_skel's geometry, batched: J spheres of radius r_joint at the joints, then L cylinders of radius r_limb from
// joint limbs[l][0] to joint limbs[l][1].  One thread per output vertex.
__global__ __launch_bounds__(kShadeWG) void skeleton_mesh_kernel(const float* __restrict__ joints, int N, int J,
                                                                 const float* __restrict__ sphere, int Vs,
                                                                 const float* __restrict__ cyl, int Vc, const int* __restrict__ limbs,
                                                                 int L, float r_joint, float r_limb,
                                                                 const unsigned char* __restrict__ hide, float* __restrict__ out) {
    const long long per = (long long)J * Vs + (long long)L * Vc;
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= (long long)N * per) return;
    const int n = (int)(i / per);
    const long long k = i - (long long)n * per;
    const float* jn = joints + (size_t)n * J * 3;
    const unsigned char* hn = hide ? hide + (size_t)n * (J + L) : nullptr;
    float* o = out + i * 3;
    if (k < (long long)J * Vs) {
        const int j = (int)(k / Vs);
        const float* t = sphere + (size_t)(k - (long long)j * Vs) * 3;
        const float* c = jn + j * 3;
        const float r = (hn && hn[j]) ? 0.f : r_joint;
        o[0] = c[0] + r * t[0], o[1] = c[1] + r * t[1], o[2] = c[2] + r * t[2];
        return;
    }
    const long long kc = k - (long long)J * Vs;
    const int l = (int)(kc / Vc);
    const float* t = cyl + (size_t)(kc - (long long)l * Vc) * 3;
    int j1 = limbs[2 * l], j2 = limbs[2 * l + 1];
    const bool bad = j1 < 0 || j1 >= J || j2 < 0 || j2 >= J;
    if (bad) j1 = 0, j2 = 0;
    const float* p1 = jn + j1 * 3;
    const float* p2 = jn + j2 * 3;
    float a[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const float len = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (bad || (hn && hn[J + l]) || !(len > 0.f) || !(len < 3.0e38f)) {
        o[0] = p1[0], o[1] = p1[1], o[2] = p1[2];
        return;
    }
    a[0] /= len, a[1] /= len, a[2] /= len;
    // u = normalise(a x e), e the coordinate axis with the smallest |a . e| (ties: the lowest index); w = a x u
    int e = 0;
    if (fabsf(a[1]) < fabsf(a[e])) e = 1;
    if (fabsf(a[2]) < fabsf(a[e])) e = 2;
    float u[3];
    if (e == 0) u[0] = 0.f, u[1] = a[2], u[2] = -a[1];
    else if (e == 1) u[0] = -a[2], u[1] = 0.f, u[2] = a[0];
    else u[0] = a[1], u[1] = -a[0], u[2] = 0.f;
    const float ul = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    u[0] /= ul, u[1] /= ul, u[2] /= ul;
    const float w[3] = {a[1] * u[2] - a[2] * u[1], a[2] * u[0] - a[0] * u[2], a[0] * u[1] - a[1] * u[0]};
    const float cx = r_limb * t[0], cy = r_limb * t[1], cz = len * t[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = p1[c] + ((cx * u[c] + cy * w[c]) + cz * a[c]);      // the small terms first: one rounding at p1's size
}

// ---- image arithmetic on uint8 images ---------------------------------------------------------------------------------
// render_img (render_util.py:161-167) per RGBA pixel: x.astype(float32) / 255.0, alpha channel times `alpha`, then
// (x * 255).astype(uint8), which truncates.
__global__ __launch_bounds__(kShadeWG) void requantize_kernel(const uchar4* __restrict__ in, float alpha, long long n,
                                                              uchar4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= n) return;
    const uchar4 p = in[i];
    const float r = __fdiv_rn((float)p.x, 255.f), g = __fdiv_rn((float)p.y, 255.f), b = __fdiv_rn((float)p.z, 255.f);
    const float a = __fdiv_rn((float)p.w, 255.f) * alpha;
    out[i] = make_uchar4((unsigned char)(int)(r * 255.f), (unsigned char)(int)(g * 255.f), (unsigned char)(int)(b * 255.f),
                         (unsigned char)(int)(a * 255.f));
}

// PIL's Image.paste(src, (0, 0), src) with an RGBA source as its own mask, on every channel of an RGB or RGBA destination:
// t = src a + dst (255 - a) + 128, out = (t + (t >> 8)) >> 8.
__global__ __launch_bounds__(kShadeWG) void paste_kernel(unsigned char* __restrict__ dst, int C, const uchar4* __restrict__ src,
                                                         long long n) {
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= n) return;
    const uchar4 s = src[i];
    const unsigned sv[4] = {s.x, s.y, s.z, s.w};
    const unsigned a = s.w;
    unsigned char* d = dst + i * C;
    for (int c = 0; c < C; ++c) {
        const unsigned t = sv[c] * a + (unsigned)d[c] * (255u - a) + 128u;
        d[c] = (unsigned char)((t + (t >> 8)) >> 8);
    }
}

// render_img_overlay (render_util.py:169-174): the source's rgb where its alpha > 0, the destination elsewhere.
__global__ __launch_bounds__(kShadeWG) void overlay_kernel(const unsigned char* __restrict__ dst, const uchar4* __restrict__ src,
                                                           long long n, unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= n) return;
    const uchar4 s = src[i];
    const bool on = s.w > 0;
    out[i * 3 + 0] = on ? s.x : dst[i * 3 + 0];
    out[i * 3 + 1] = on ? s.y : dst[i * 3 + 1];
    out[i * 3 + 2] = on ? s.z : dst[i * 3 + 2];
}

// Image.FLIP_LEFT_RIGHT on `rows` rows of W pixels of C bytes
__global__ __launch_bounds__(kShadeWG) void flip_lr_kernel(const unsigned char* __restrict__ in, long long rows, int W, int C,
                                                           unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kShadeWG + threadIdx.x;
    if (i >= rows * W) return;
    const long long row = i / W;
    const int x = (int)(i - row * W);
    const unsigned char* s = in + (row * W + (W - 1 - x)) * C;
    unsigned char* d = out + i * C;
    for (int c = 0; c < C; ++c) d[c] = s[c];
}

static unsigned grid_for(long long n) { return (unsigned)((n + kShadeWG - 1) / kShadeWG); }

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_vertex_normals(const float* verts, const int* faces, const int* offsets, const int* face_ids, int n_mesh, int V,
                                   int F, float* normals, rohm_stream_t stream) {
    ROHM_ARG_CHECK(verts && faces && offsets && face_ids && normals, "vertex_normals: null argument");
    ROHM_ARG_CHECK(n_mesh > 0 && V > 0 && F > 0, "vertex_normals: need n_mesh, V, F > 0 (got %d, %d, %d)", n_mesh, V, F);
    const long long n = (long long)n_mesh * V;
    ROHM_ARG_CHECK(n < (1ll << 31) && (long long)F * 3 < (1ll << 31), "vertex_normals: batch too large: split the call");
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(grid_for(n)), dim3(kShadeWG), 0, (hipStream_t)stream, verts, faces, offsets,
                       face_ids, n_mesh, V, F, normals);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" size_t rohm_color_workspace_bytes(int n_mesh, int F, int W, int H) {
    return rohm_depth_workspace_bytes(n_mesh, F, W, H);
}

extern "C" int rohm_color_render(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform, double fx,
                                 double fy, double cx, double cy, int W, int H, double znear, double zfar, int cull_backfaces,
                                 const float* normals, const unsigned char* colors, int colors_per_mesh, float ambient, float diffuse,
                                 unsigned char* rgba, float* depth, int* face_id, void* ws, size_t ws_bytes, rohm_stream_t stream) {
    ROHM_ARG_CHECK(verts && faces && colors && rgba && ws, "color_render: null argument");
    ROHM_ARG_CHECK(n_mesh > 0 && V > 0 && F > 0, "color_render: need n_mesh, V, F > 0 (got %d, %d, %d)", n_mesh, V, F);
    if (int rc = check_camera("color_render", fx, fy, W, H, znear, zfar)) return rc;
    const long long nt = (long long)n_mesh * F;
    const int tiles_x = (W + kTile - 1) / kTile, n_tiles = tiles_x * ((H + kTile - 1) / kTile);
    const long long n_mt = (long long)n_mesh * n_tiles;
    ROHM_ARG_CHECK(nt * kBinSpan < (1ll << 31) && n_mt < (1ll << 31) && (long long)n_mesh * V < (1ll << 31),
                   "color_render: batch too large (%d meshes x %d faces): split the call", n_mesh, F);
    size_t need = 0;
    RenderWs w = carve(ws, n_mesh, nt, n_mt, &need);
    if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        set_error("color_render: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", need, ws_bytes);
        return ROHM_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Camera cam{fx, fy, cx, cy, znear, zfar, W, H};
    const Xform xf = make_xform(transform);
    prof::Scope ps("color_render", 60.0 * nt, (double)sizeof(TriRec) * 2 * nt + 12.0 * n_mesh * W * H, s);
    if (int rc = bin_triangles(verts, faces, n_mesh, V, F, xf, cam, cull_backfaces, tiles_x, n_tiles, w, s)) return rc;
    const ShadeArgs a{verts, faces, normals, colors, V, colors_per_mesh != 0, cull_backfaces != 0, ambient, diffuse, rgba, depth, face_id};
    hipLaunchKernelGGL(shade_tile_kernel, dim3((unsigned)n_mt), dim3(kRasterWG), 0, s, a, xf, F, cam, tiles_x, n_tiles, w);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_skeleton_mesh(const float* joints, int N, int J, const float* sphere, int Vs, const float* cylinder, int Vc,
                                  const int* limbs, int L, float r_joint, float r_limb, const unsigned char* hide, float* verts,
                                  rohm_stream_t stream) {
    ROHM_ARG_CHECK(joints && sphere && cylinder && limbs && verts, "skeleton_mesh: null argument");
    ROHM_ARG_CHECK(N > 0 && J > 0 && L > 0 && Vs > 0 && Vc > 0, "skeleton_mesh: need N, J, L, Vs, Vc > 0");
    const long long n = (long long)N * ((long long)J * Vs + (long long)L * Vc);
    ROHM_ARG_CHECK(n < (1ll << 31), "skeleton_mesh: batch too large: split the call");
    hipLaunchKernelGGL(skeleton_mesh_kernel, dim3(grid_for(n)), dim3(kShadeWG), 0, (hipStream_t)stream, joints, N, J, sphere, Vs,
                       cylinder, Vc, limbs, L, r_joint, r_limb, hide, verts);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_image_requantize(const unsigned char* rgba, float alpha, long long n_pixels, unsigned char* out,
                                     rohm_stream_t stream) {
    ROHM_ARG_CHECK(rgba && out && n_pixels > 0 && n_pixels < (1ll << 39), "image_requantize: null or empty argument");
    hipLaunchKernelGGL(requantize_kernel, dim3(grid_for(n_pixels)), dim3(kShadeWG), 0, (hipStream_t)stream, (const uchar4*)rgba, alpha,
                       n_pixels, (uchar4*)out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_image_paste(unsigned char* dst, int dst_channels, const unsigned char* src_rgba, long long n_pixels,
                                rohm_stream_t stream) {
    ROHM_ARG_CHECK(dst && src_rgba && n_pixels > 0 && n_pixels < (1ll << 39), "image_paste: null or empty argument");
    ROHM_ARG_CHECK(dst_channels == 3 || dst_channels == 4, "image_paste: the destination is RGB or RGBA (got %d channels)", dst_channels);
    hipLaunchKernelGGL(paste_kernel, dim3(grid_for(n_pixels)), dim3(kShadeWG), 0, (hipStream_t)stream, dst, dst_channels,
                       (const uchar4*)src_rgba, n_pixels);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_image_overlay(const unsigned char* dst_rgb, const unsigned char* src_rgba, long long n_pixels, unsigned char* out,
                                  rohm_stream_t stream) {
    ROHM_ARG_CHECK(dst_rgb && src_rgba && out && n_pixels > 0 && n_pixels < (1ll << 39), "image_overlay: null or empty argument");
    hipLaunchKernelGGL(overlay_kernel, dim3(grid_for(n_pixels)), dim3(kShadeWG), 0, (hipStream_t)stream, dst_rgb, (const uchar4*)src_rgba,
                       n_pixels, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_image_flip_lr(const unsigned char* in, long long rows, int W, int channels, unsigned char* out,
                                  rohm_stream_t stream) {
    ROHM_ARG_CHECK(in && out && in != out && rows > 0 && W > 0 && channels > 0 && channels <= 4, "image_flip_lr: bad argument");
    ROHM_ARG_CHECK(rows * W < (1ll << 39), "image_flip_lr: image too large");
    hipLaunchKernelGGL(flip_lr_kernel, dim3(grid_for(rows * W)), dim3(kShadeWG), 0, (hipStream_t)stream, in, rows, W, channels, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
