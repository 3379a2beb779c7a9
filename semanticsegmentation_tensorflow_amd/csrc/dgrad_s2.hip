// dgrad_s2: Conv2DBackpropInput of a 4x4 stride-2 Conv2D (the encoder convs
// of Network/model/LidCamNet.py:34-38) as one halo kernel per tile, bf16 / f16
// with fp32 accumulation.
//
//   dx[n][ih][iw][c] = sum_{r,s,k} dy[n][oh][ow][k] W[r][s][c][k],
//   2 oh + r = ih + pad_top, 2 ow + s = iw + pad_left
//
// One block (4 waves) owns an 8 x 32 tile of dx in padded coordinates whose
// origin is even, i.e. 4 x 16 pixels of each of the 4 stride phases, and 32
// dx channels (blockIdx.y).  It stages the tile's dy halo -- 5 x 17 pixels x K
// channels -- once in LDS with the buffer-resource LDS DMA (pixels outside the
// map, the pad chunk of every row and the tail of the last 1 KiB piece land as
// zeros through the resource's bounds), then wave w = phase (w >> 1, w & 1)
// runs its 4 taps x K/32 steps of v_mfma_f32_16x16x32 from that one halo:
// A = W[r][s][c0 .. c0+15][k .. k+31] read from the HWIO copy (k-contiguous,
// 16 bytes per lane straight from global memory: every wave has its own four
// taps, so LDS would not share them), B = 16 pixels of one phase row from the
// halo.  The accumulator has the pixel on the lane and 4 consecutive channels
// in its registers: each dx element is written once, by 8-byte vector stores.
// No atomics, no split-K, no workspace.  Index math: dgrad_s2_geom.h.
#include "common.h"
#include "igemm.h"
#include "ldsdma.h"
#include "dgrad_s2_geom.h"

namespace seg {

static_assert((dg2::HPIX * (dg2::KMAX / 8 + 1) + 63) / 64 * 1024 <= 160 * 1024, "dy halo fits the CU's LDS");
static_assert((dg2::HPIX * (dg2::KMAX / 8 + 1) + 63) / 64 * 1024 <= 64 * 1024, "dynamic LDS without opt-in");

struct Dg2Params {
    const void* dy;
    const void* w;
    void* dx;
    const void* res;
    const void* mask;
    int H, W, C, OH, OW, K;
    int ldx, ldy, ld_res, ld_mask;
    int pad_t, pad_l, c_valid;
    int tiles_x, tiles_y, wrow;
    float mask_scale;
};

template <typename T> struct alignas(8) Quad { T v[4]; };

template <typename T, int NCT>
__global__ __launch_bounds__(256) void dgrad_s2_k(Dg2Params p) {
    extern __shared__ __attribute__((aligned(16))) char dg2_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tpi = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tpi;
    const int trem = blockIdx.x - img * tpi;
    const int ty = trem / p.tiles_x, tx = trem - (trem / p.tiles_x) * p.tiles_x;
    const int u0 = ty * dg2::TH, v0 = tx * dg2::TW;
    const int cb0 = blockIdx.y * dg2::CB;

    // ---- the dy halo, once ----
    const T* dyi = reinterpret_cast<const T*>(p.dy) + (long)img * p.OH * p.OW * p.ldy;
    const seg_i32x4 rs = make_rsrc(dyi, (unsigned)((((long)p.OH * p.OW - 1) * p.ldy + p.K) * 2));
    const unsigned lds0 = (unsigned)(uintptr_t)(SEG_LDS char*)dg2_smem;
    const int npieces = dg2::lds_bytes(p.K) / 1024;
    for (int pc = w; pc < npieces; pc += 4)
        bglds16(rs, dg2::halo_src(pc * 64 + lane, u0, v0, p.OH, p.OW, p.ldy, p.K), 0u, lds0 + (unsigned)pc * 1024u);
    wait_vmcnt<0>();
    __syncthreads();

    // ---- 4 taps x K/32 steps of this wave's phase ----
    const int ph = w >> 1, pw = w & 1;
    const int fr = lane & 15, fg = lane >> 4;
    const int rowb = dg2::row_chunks(p.K) * 16;          // LDS bytes of one halo pixel
    const int ksteps = p.K / 32;
    f32x4 acc[dg2::PH][NCT];
#pragma unroll
    for (int i = 0; i < dg2::PH; ++i)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[i][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const T* __restrict__ Wg = reinterpret_cast<const T*>(p.w);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int jr = t >> 1, js = t & 1;
        const int r = ph + 2 * jr, s = pw + 2 * js;
        const T* wt = Wg + (long)((r * dg2::S + s) * p.C + cb0 + fr) * p.wrow + fg * 8;
        const char* ap = dg2_smem + dg2::halo_pix(0, fr, jr, js) * rowb + fg * 16;
        for (int kk = 0; kk < ksteps; ++kk) {
            uint4 wf[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                wf[ct] = *reinterpret_cast<const uint4*>(wt + (long)ct * 16 * p.wrow + kk * 32);
#pragma unroll
            for (int i = 0; i < dg2::PH; ++i) {
                const uint4 a = *reinterpret_cast<const uint4*>(ap + i * dg2::HWD * rowb + kk * 64);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[i][ct] = mfma16x16x32<T>(wf[ct], a, acc[i][ct]);
            }
        }
    }

    // ---- epilogue: lane = pixel fr of each phase row, 4 channels per register quad ----
    T* __restrict__ dx = reinterpret_cast<T*>(p.dx);
    const T* __restrict__ res = reinterpret_cast<const T*>(p.res);
    const T* __restrict__ mask = reinterpret_cast<const T*>(p.mask);
    const int iw = dg2::slot_iw(v0, pw, fr, p.pad_l);
#pragma unroll
    for (int i = 0; i < dg2::PH; ++i) {
        const int ih = dg2::slot_ih(u0, ph, i, p.pad_t);
        if ((unsigned)ih >= (unsigned)p.H || (unsigned)iw >= (unsigned)p.W) continue;
        const long pix = ((long)img * p.H + ih) * p.W + iw;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int c = cb0 + ct * 16 + fg * 4;
            float v[4] = {acc[i][ct][0], acc[i][ct][1], acc[i][ct][2], acc[i][ct][3]};
            if (res) {
                const Quad<T> q = *reinterpret_cast<const Quad<T>*>(res + pix * p.ld_res + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += to_f32(q.v[e]);
            }
            if (mask) {
                const Quad<T> q = *reinterpret_cast<const Quad<T>*>(mask + pix * p.ld_mask + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = to_f32(q.v[e]) > 0.f ? v[e] * p.mask_scale : 0.f;
            }
            Quad<T> o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o.v[e] = from_f32<T>(c + e < p.c_valid ? v[e] : 0.f);
            *reinterpret_cast<Quad<T>*>(dx + pix * p.ldx + c) = o;
        }
    }
}

bool dgrad_s2_shape_ok(const seg_conv_desc* d) {
    return dg2::shape_ok(d->N, d->H, d->W, d->C, d->OH, d->OW, d->K, d->R, d->S, d->stride_h, d->stride_w, d->dil_h,
                         d->dil_w, d->pad_top, d->pad_left, d->ldx, d->ldy);
}

int launch_dgrad_s2(const seg_conv_desc* d, const void* dy, const void* w_hwio, const seg_epilogue* epi, void* dx,
                    int wpad, hipStream_t s) {
    if ((d->dtype != SEG_BF16 && d->dtype != SEG_F16) || !dgrad_s2_shape_ok(d)) return SEG_EINVAL;
    if (((uintptr_t)dy | (uintptr_t)w_hwio | (uintptr_t)dx) & 15) return SEG_EALIGN;
    Dg2Params p = {};
    p.dy = dy; p.w = w_hwio; p.dx = dx;
    p.H = d->H; p.W = d->W; p.C = d->C; p.OH = d->OH; p.OW = d->OW; p.K = d->K;
    p.ldx = d->ldx; p.ldy = d->ldy;
    p.pad_t = d->pad_top; p.pad_l = d->pad_left; p.c_valid = d->c_valid;
    p.tiles_x = dg2::tiles_x(d->W, d->pad_left); p.tiles_y = dg2::tiles_y(d->H, d->pad_top);
    p.wrow = d->K + wpad;
    p.mask_scale = 1.f;
    if (epi) {
        if (epi->residual) {
            p.res = epi->residual;
            p.ld_res = epi->ld_residual ? epi->ld_residual : d->ldx;
            if ((p.ld_res & 3) || ((uintptr_t)p.res & 7)) return SEG_EALIGN;
        }
        if (epi->relu_mask) {
            p.mask = epi->relu_mask;
            p.ld_mask = epi->ld_relu_mask > 0 ? epi->ld_relu_mask : d->ldx;
            p.mask_scale = epi->mask_scale != 0.f ? epi->mask_scale : 1.f;
            if ((p.ld_mask & 3) || ((uintptr_t)p.mask & 7)) return SEG_EALIGN;
        }
    }
    const dim3 grid((unsigned)(d->N * p.tiles_x * p.tiles_y), (unsigned)((d->C + dg2::CB - 1) / dg2::CB));
    const size_t lds = (size_t)dg2::lds_bytes(d->K);
#define DG2_LAUNCH(T, NCT) hipLaunchKernelGGL((dgrad_s2_k<T, NCT>), grid, dim3(256), lds, s, p)
    if (d->dtype == SEG_BF16) {
        if (d->C == 16) DG2_LAUNCH(bf16, 1); else DG2_LAUNCH(bf16, 2);
    } else {
        if (d->C == 16) DG2_LAUNCH(f16, 1); else DG2_LAUNCH(f16, 2);
    }
#undef DG2_LAUNCH
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

}  // namespace seg
