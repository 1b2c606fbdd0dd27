// batch_kernels.hip -- one training batch of SceneDataset.__getitem__ + collate_fn (reference code/datasets/scene_dataset.py:107-203) assembled on the
// device from pools that stay there for the whole run (mvsdf_amd/datasets/device_batches.py).  One launch per step, no host wait.
//
// Grid: blockIdx.y < B (1 + num_src) = one feature map each (the bulk of the bytes: a contiguous block of 32 fh fw floats in channels-last storage,
// copied with 16-byte loads and stores, BT_UNROLL in flight per thread); blockIdx.y == B (1 + num_src) = everything else (sampled pixels, depth maps,
// cameras), grid-strided over the same blockIdx.x range.
#include <hip/hip_runtime.h>
#include "capi_util.h"

#define BT_THREADS 256
#define BT_UNROLL 4

static __device__ __forceinline__ bool bt_view_ok(int64_t v, int n) { return v >= 0 && v < n; }

__global__ void __launch_bounds__(BT_THREADS) k_batch_gather(MvsdfBatchArgs a) {
    const int V1 = 1 + a.num_src;
    const int job = blockIdx.y;
    if (job < a.B * V1) {
        const int b = job / V1, k = job - b * V1;
        const int64_t v = a.views[b];
        if (!bt_view_ok(v, a.n)) return;
        const int64_t sv = k == 0 ? v : a.src[v * a.num_src + (k - 1)];
        if (!bt_view_ok(sv, a.n)) return;
        const int64_t m4 = a.fmap_floats / 4;
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(a.feats + sv * a.fmap_floats);
        float4* __restrict__ d4 = reinterpret_cast<float4*>(k == 0 ? a.o_feat + (int64_t)b * a.fmap_floats
                                                                   : a.o_feat_src + ((int64_t)b * a.num_src + (k - 1)) * a.fmap_floats);
        const int64_t stride = (int64_t)gridDim.x * BT_THREADS * BT_UNROLL;
        for (int64_t base = (int64_t)blockIdx.x * BT_THREADS * BT_UNROLL + threadIdx.x; base < m4; base += stride) {
            float4 r[BT_UNROLL];
#pragma unroll
            for (int u = 0; u < BT_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * BT_THREADS;
                if (i < m4) r[u] = s4[i];
            }
#pragma unroll
            for (int u = 0; u < BT_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * BT_THREADS;
                if (i < m4) d4[i] = r[u];
            }
        }
        return;
    }
    // the rest: B P sampled pixels, then B depth maps, then per view 100 + 32 num_src camera floats, 4 scene floats
    const int64_t n_pix = (int64_t)a.B * a.P;
    const int64_t n_dep = (int64_t)a.B * a.depth_floats;
    const int per_view = 16 + 16 + 32 + 32 + 32 * a.num_src + 4;
    const int64_t total = n_pix + n_dep + (int64_t)a.B * per_view;
    for (int64_t t = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * BT_THREADS) {
        if (t < n_pix) {
            const int b = (int)(t / a.P);
            const int64_t p = t - (int64_t)b * a.P;
            const int64_t v = a.views[b];
            const int64_t id = a.pix ? a.pix[p] : p;
            if (!bt_view_ok(v, a.n) || id < 0 || id >= a.total_pixels) continue;
            const int64_t q = v * a.total_pixels + id;
            a.o_rgb[t * 3 + 0] = a.rgb[q * 3 + 0];
            a.o_rgb[t * 3 + 1] = a.rgb[q * 3 + 1];
            a.o_rgb[t * 3 + 2] = a.rgb[q * 3 + 2];
            const int64_t y = id / a.img_w;
            a.o_uv[t * 2 + 0] = (float)(id - y * a.img_w);      // x = id mod W, y = id div W: the reference's flipped mgrid (scene_dataset.py:88-90)
            a.o_uv[t * 2 + 1] = (float)y;
            a.o_omask[t] = a.omask[q];
            if (a.pmask && a.o_pmask) a.o_pmask[t] = a.pmask[q];
            continue;
        }
        int64_t r = t - n_pix;
        if (r < n_dep) {
            const int b = (int)(r / a.depth_floats);
            const int64_t v = a.views[b];
            if (bt_view_ok(v, a.n)) a.o_depths[r] = a.depths[v * a.depth_floats + (r - (int64_t)b * a.depth_floats)];
            continue;
        }
        r -= n_dep;
        const int b = (int)(r / per_view);
        int e = (int)(r - (int64_t)b * per_view);
        const int64_t v = a.views[b];
        if (!bt_view_ok(v, a.n)) continue;
        if (e < 16) { a.o_pose[b * 16 + e] = a.pose[v * 16 + e]; continue; }
        e -= 16;
        if (e < 16) { a.o_intrinsics[b * 16 + e] = a.intrinsics[v * 16 + e]; continue; }
        e -= 16;
        if (e < 32) { a.o_cam[b * 32 + e] = a.cams_hd[v * 32 + e]; continue; }
        e -= 32;
        if (e < 32) { a.o_depth_cams[b * 32 + e] = a.depth_cams[v * 32 + e]; continue; }
        e -= 32;
        if (e < 32 * a.num_src) {
            const int s = e / 32;
            const int64_t sv = a.src[v * a.num_src + s];
            if (bt_view_ok(sv, a.n)) a.o_src_cams[((int64_t)b * a.num_src + s) * 32 + (e - s * 32)] = a.cams_hd[sv * 32 + (e - s * 32)];
            continue;
        }
        e -= 32 * a.num_src;
        if (e == 0) a.o_size[b] = a.size[0];
        else a.o_center[b * 3 + (e - 1)] = a.center[e - 1];
    }
}

static bool bt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

size_t mvsdf_batch_args_bytes(void) { return sizeof(MvsdfBatchArgs); }

int mvsdf_batch_gather(const MvsdfBatchArgs* ap, void* stream) {
    if (!ap) return mv_fail(-1, "mvsdf_batch_gather: no arguments");
    const MvsdfBatchArgs& a = *ap;
    if (a.B < 1 || a.n < 1 || a.num_src < 0 || a.P < 1 || a.img_w < 1 || a.total_pixels < 1 || a.depth_floats < 1 || a.fmap_floats < 4 ||
        a.fmap_floats % 4 || a.total_pixels % a.img_w || (!a.pix && a.P != a.total_pixels) || (int64_t)a.B * (1 + a.num_src) >= 65535)
        return mv_fail(-1, "mvsdf_batch_gather: bad sizes");
    if (!a.views || (a.num_src && !a.src) || !a.rgb || !a.omask || !a.pose || !a.intrinsics || !a.cams_hd || !a.depth_cams || !a.depths || !a.size ||
        !a.center || !a.feats || !a.o_rgb || !a.o_uv || !a.o_omask || (a.pmask && !a.o_pmask) || !a.o_pose || !a.o_intrinsics || !a.o_cam ||
        (a.num_src && !a.o_src_cams) || !a.o_depths || !a.o_depth_cams || !a.o_size || !a.o_center || !a.o_feat || (a.num_src && !a.o_feat_src))
        return mv_fail(-1, "mvsdf_batch_gather: missing pointer");
    if (!bt_aligned16(a.feats) || !bt_aligned16(a.o_feat) || (a.num_src && !bt_aligned16(a.o_feat_src)))
        return mv_fail(-1, "mvsdf_batch_gather: feature maps must be 16-byte aligned");
    const int64_t m4 = a.fmap_floats / 4;
    int64_t gx = (m4 + BT_THREADS * BT_UNROLL - 1) / (BT_THREADS * BT_UNROLL);
    const int64_t rest = (int64_t)a.B * a.P + (int64_t)a.B * a.depth_floats;
    const int64_t gr = (rest + BT_THREADS - 1) / BT_THREADS;
    if (gr > gx) gx = gr;
    if (gx > 4096) gx = 4096;                                    // both roles grid-stride: 4096 x 256 threads cover the chip many times over
    hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)gx, (unsigned)(a.B * (1 + a.num_src) + 1)), dim3(BT_THREADS), 0, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mvsdf_batch_gather");
}

}  // extern "C"
