// General windowed pooling (any window, stride, TF SAME / VALID) and constant
// zero padding on H and W: PSPNet50's 3x3 stride-2 max pool, its pyramid's
// anisotropic average pools and its tf.pad (Network/model/PSPNet.py:30-34,
// :147-166; Network/utils/utils.py:306-310, :325-327).  HBM- or latency-bound:
// 16-byte chunks per lane, grid-stride loops, 32-bit index math (the host
// checks the counts), fp32 sums rounded once.  The gradients are gathers --
// one thread per input pixel and chunk over the windows that contain it -- so
// there are no atomics, no memset, and dx is written whole.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ uint4 ldc(const T* p) { return *reinterpret_cast<const uint4*>(p); }
template <typename T>
__device__ __forceinline__ void stc(T* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }

constexpr int POOL_MAX = 0, POOL_AVG = 1;

// In-image extent of window `o` along one axis: rows [lo, hi) of the window.
__device__ __forceinline__ void win_range(int o, int stride, int pad, int k, int in, int& lo, int& hi) {
    const int start = o * stride - pad;
    lo = start < 0 ? -start : 0;
    hi = in - start < k ? in - start : k;
}

// One thread per (pooled pixel, chunk).  Max: the in-image maximum and, with
// idx, the row-major window position r * kw + s of its first occurrence
// (strict '>': TF's tie rule, as maxpool_fwd_idx_k).  Avg: row sums added row
// by row, divided by the number of in-image elements.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void pool_fwd_k(seg_pool_desc d, const T* __restrict__ x, T* __restrict__ y,
                                                  unsigned char* __restrict__ idx, unsigned CK, unsigned total) {
    constexpr int EPC = dt_traits<T>::EPC;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned cc = i % CK, pix = i / CK;
        const unsigned ow = pix % (unsigned)d.OW, t = pix / (unsigned)d.OW;
        const unsigned oh = t % (unsigned)d.OH, n = t / (unsigned)d.OH;
        int r0, r1, s0, s1;
        win_range((int)oh, d.sh, d.pad_top, d.kh, d.H, r0, r1);
        win_range((int)ow, d.sw, d.pad_left, d.kw, d.W, s0, s1);
        const int ih0 = (int)oh * d.sh - d.pad_top, iw0 = (int)ow * d.sw - d.pad_left;
        float acc[EPC];
        unsigned arg[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) { acc[e] = 0.f; arg[e] = 0u; }
        bool first = true;
        for (int r = r0; r < r1; ++r) {
            const T* row = x + ((long)(n * (unsigned)d.H + (unsigned)(ih0 + r)) * d.W + iw0) * d.ldx + cc * EPC;
            float ra[EPC];
            for (int s = s0; s < s1; ++s) {
                float v[EPC];
                Chunk<T>::unpack(ldc(row + (long)s * d.ldx), v);
                if constexpr (KIND == POOL_MAX) {
                    const unsigned pos = (unsigned)(r * d.kw + s);
#pragma unroll
                    for (int e = 0; e < EPC; ++e)
                        if (first || v[e] > acc[e]) { acc[e] = v[e]; arg[e] = pos; }
                    first = false;
                } else {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) ra[e] = s == s0 ? v[e] : ra[e] + v[e];
                }
            }
            if constexpr (KIND == POOL_AVG) {
                if (s0 < s1) {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] = first ? ra[e] : acc[e] + ra[e];
                    first = false;
                }
            }
        }
        if constexpr (KIND == POOL_AVG) {
            const float cnt = (float)((r1 - r0) * (s1 - s0));
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = first ? 0.f : acc[e] / cnt;
        }
        stc(y + (long)pix * d.ldy + cc * EPC, Chunk<T>::pack(acc));
        if constexpr (KIND == POOL_MAX) {
            if (idx) {
                unsigned long long code = 0;
#pragma unroll
                for (int e = 0; e < EPC; ++e) code |= (unsigned long long)(arg[e] & 0xffu) << (8 * e);
                unsigned char* q = idx + (long)pix * d.C + cc * EPC;
                if constexpr (EPC == 8) *reinterpret_cast<unsigned long long*>(q) = code;
                else *reinterpret_cast<unsigned*>(q) = (unsigned)code;
            }
        }
    }
}

// Windows o along one axis that contain input coordinate `in`: [lo, hi].
__device__ __forceinline__ void cover_range(int in, int stride, int pad, int k, int out, int& lo, int& hi) {
    const int t = in + pad - k + 1;
    lo = t <= 0 ? 0 : (t + stride - 1) / stride;
    hi = (in + pad) / stride;
    if (hi > out - 1) hi = out - 1;
}

// One thread per (input pixel, chunk): the sum, in window order, of dy where
// the window's switch names this pixel (max) or of dy / count (avg).  A pixel
// no window covers (VALID leftovers, the gaps of k < s) gets 0.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void pool_bwd_k(seg_pool_desc d, const unsigned char* __restrict__ idx,
                                                  const T* __restrict__ dy, T* __restrict__ dx, unsigned CK,
                                                  unsigned total) {
    constexpr int EPC = dt_traits<T>::EPC;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned cc = i % CK, pix = i / CK;
        const unsigned iw = pix % (unsigned)d.W, t = pix / (unsigned)d.W;
        const unsigned ih = t % (unsigned)d.H, n = t / (unsigned)d.H;
        int oh0, oh1, ow0, ow1;
        cover_range((int)ih, d.sh, d.pad_top, d.kh, d.OH, oh0, oh1);
        cover_range((int)iw, d.sw, d.pad_left, d.kw, d.OW, ow0, ow1);
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        unsigned has = 0u;                    // elements that already hold a contribution
        for (int oh = oh0; oh <= oh1; ++oh) {
            const int r = (int)ih + d.pad_top - oh * d.sh;
            int r0, r1;
            win_range(oh, d.sh, d.pad_top, d.kh, d.H, r0, r1);
            for (int ow = ow0; ow <= ow1; ++ow) {
                const int s = (int)iw + d.pad_left - ow * d.sw;
                const unsigned opix = (n * (unsigned)d.OH + (unsigned)oh) * (unsigned)d.OW + (unsigned)ow;
                float g[EPC];
                Chunk<T>::unpack(ldc(dy + (long)opix * d.ldy + cc * EPC), g);
                if constexpr (KIND == POOL_MAX) {
                    const unsigned char* q = idx + (long)opix * d.C + cc * EPC;
                    unsigned long long code;
                    if constexpr (EPC == 8) code = *reinterpret_cast<const unsigned long long*>(q);
                    else code = *reinterpret_cast<const unsigned*>(q);
                    const unsigned pos = (unsigned)(r * d.kw + s);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        if (((unsigned)(code >> (8 * e)) & 0xffu) == pos) {
                            acc[e] = (has >> e) & 1u ? acc[e] + g[e] : g[e];
                            has |= 1u << e;
                        }
                    }
                } else {
                    int s0, s1;
                    win_range(ow, d.sw, d.pad_left, d.kw, d.W, s0, s1);
                    const float cnt = (float)((r1 - r0) * (s1 - s0));
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] = has ? acc[e] + g[e] / cnt : g[e] / cnt;
                    has = 1u;
                }
            }
        }
        stc(dx + (long)pix * d.ldx + cc * EPC, Chunk<T>::pack(acc));
    }
}

// y[n, h, w] = x[n, h - top, w - left] inside x, 0 outside: tf.pad with
// (top, left) >= 0, its gradient (the crop) with (top, left) <= 0.  One thread
// per (y pixel, chunk).
template <typename T>
__global__ __launch_bounds__(256) void shift_copy_k(const T* __restrict__ x, int ldx, int XH, int XW,
                                                    T* __restrict__ y, int ldy, unsigned YH, unsigned YW, int top,
                                                    int left, unsigned CK, unsigned total) {
    constexpr int EPC = dt_traits<T>::EPC;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned cc = i % CK, pix = i / CK;
        const unsigned w = pix % YW, t = pix / YW;
        const unsigned h = t % YH, n = t / YH;
        const int xh = (int)h - top, xw = (int)w - left;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (xh >= 0 && xh < XH && xw >= 0 && xw < XW)
            v = ldc(x + ((long)(n * (unsigned)XH + (unsigned)xh) * XW + xw) * ldx + cc * EPC);
        stc(y + (long)pix * ldy + cc * EPC, v);
    }
}

inline int epc_of(int dtype) { return dtype == SEG_F32 ? 4 : 8; }
inline bool dtype_ok(int dtype) { return dtype == SEG_F32 || dtype == SEG_BF16 || dtype == SEG_F16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr long LIMIT = 1L << 31;

// TF's output size and leading pad along one axis; false when there is no output.
bool axis_geom(int in, int k, int s, int padding, int* out, int* before) {
    if (padding == 0) {
        *out = (in + s - 1) / s;
        const long total = (long)(*out - 1) * s + k - in;
        *before = total > 0 ? (int)(total / 2) : 0;
    } else {
        if (in < k) return false;
        *out = (in - k) / s + 1;
        *before = 0;
    }
    return *out >= 1;
}

// Everything a launch relies on, re-derived from the descriptor's own fields
// (a caller may have built or edited it by hand).
bool desc_ok(const seg_pool_desc* d) {
    if (!d || !dtype_ok(d->dtype) || (d->kind != POOL_MAX && d->kind != POOL_AVG)) return false;
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->C < 1 || d->kh < 1 || d->kw < 1 || d->sh < 1 || d->sw < 1 ||
        d->OH < 1 || d->OW < 1 || d->pad_top < 0 || d->pad_left < 0)
        return false;
    if ((long)d->kh * d->kw > 256) return false;
    const int epc = epc_of(d->dtype);
    if (d->C % epc || d->ldx % epc || d->ldy % epc || d->ldx < d->C || d->ldy < d->C) return false;
    if (d->pad_top >= d->kh || d->pad_left >= d->kw) return false;
    // every window holds an in-image element, and none starts past the image
    if ((long)(d->OH - 1) * d->sh - d->pad_top >= d->H || (long)(d->OW - 1) * d->sw - d->pad_left >= d->W) return false;
    if ((long)d->N * d->H * d->W * d->ldx >= LIMIT || (long)d->N * d->OH * d->OW * d->ldy >= LIMIT) return false;
    return true;
}

}  // namespace

extern "C" int seg_pool_desc_init(seg_pool_desc* d, int N, int H, int W, int C, int kh, int kw, int sh, int sw,
                                  int padding, int kind, int dtype) {
    if (!d || !dtype_ok(dtype) || (padding != 0 && padding != 1) || (kind != POOL_MAX && kind != POOL_AVG))
        return SEG_EINVAL;
    if (N < 1 || H < 1 || W < 1 || C < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1) return SEG_EINVAL;
    if ((long)kh * kw > 256 || C % epc_of(dtype)) return SEG_EINVAL;
    seg_pool_desc t;
    t.N = N; t.H = H; t.W = W; t.C = C;
    t.kh = kh; t.kw = kw; t.sh = sh; t.sw = sw;
    if (!axis_geom(H, kh, sh, padding, &t.OH, &t.pad_top) || !axis_geom(W, kw, sw, padding, &t.OW, &t.pad_left))
        return SEG_EINVAL;
    t.ldx = C; t.ldy = C;
    t.kind = kind; t.dtype = dtype;
    if (!desc_ok(&t)) return SEG_EINVAL;
    *d = t;
    return SEG_OK;
}

extern "C" int seg_pool2d_fwd(const seg_pool_desc* d, const void* x, void* y, uint8_t* idx, void* stream) {
    if (!desc_ok(d) || !x || !y || !aligned16(x) || !aligned16(y) || ((uintptr_t)idx & 7)) return SEG_EINVAL;
    const unsigned CK = (unsigned)(d->C / epc_of(d->dtype));
    const long total = (long)d->N * d->OH * d->OW * CK;
    const dim3 grid(seg_grid_1d(total, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d->kind == POOL_MAX) {
        if (d->dtype == SEG_BF16)
            hipLaunchKernelGGL((pool_fwd_k<bf16, POOL_MAX>), grid, block, 0, s, *d, (const bf16*)x, (bf16*)y, idx, CK, (unsigned)total);
        else if (d->dtype == SEG_F16)
            hipLaunchKernelGGL((pool_fwd_k<f16, POOL_MAX>), grid, block, 0, s, *d, (const f16*)x, (f16*)y, idx, CK, (unsigned)total);
        else
            hipLaunchKernelGGL((pool_fwd_k<float, POOL_MAX>), grid, block, 0, s, *d, (const float*)x, (float*)y, idx, CK, (unsigned)total);
    } else {
        if (d->dtype == SEG_BF16)
            hipLaunchKernelGGL((pool_fwd_k<bf16, POOL_AVG>), grid, block, 0, s, *d, (const bf16*)x, (bf16*)y, idx, CK, (unsigned)total);
        else if (d->dtype == SEG_F16)
            hipLaunchKernelGGL((pool_fwd_k<f16, POOL_AVG>), grid, block, 0, s, *d, (const f16*)x, (f16*)y, idx, CK, (unsigned)total);
        else
            hipLaunchKernelGGL((pool_fwd_k<float, POOL_AVG>), grid, block, 0, s, *d, (const float*)x, (float*)y, idx, CK, (unsigned)total);
    }
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" int seg_pool2d_bwd(const seg_pool_desc* d, const uint8_t* idx, const void* dy, void* dx, void* stream) {
    if (!desc_ok(d) || !dy || !dx || !aligned16(dy) || !aligned16(dx)) return SEG_EINVAL;
    if (d->kind == POOL_MAX && (!idx || ((uintptr_t)idx & 7))) return SEG_EINVAL;
    const unsigned CK = (unsigned)(d->C / epc_of(d->dtype));
    const long total = (long)d->N * d->H * d->W * CK;
    const dim3 grid(seg_grid_1d(total, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d->kind == POOL_MAX) {
        if (d->dtype == SEG_BF16)
            hipLaunchKernelGGL((pool_bwd_k<bf16, POOL_MAX>), grid, block, 0, s, *d, idx, (const bf16*)dy, (bf16*)dx, CK, (unsigned)total);
        else if (d->dtype == SEG_F16)
            hipLaunchKernelGGL((pool_bwd_k<f16, POOL_MAX>), grid, block, 0, s, *d, idx, (const f16*)dy, (f16*)dx, CK, (unsigned)total);
        else
            hipLaunchKernelGGL((pool_bwd_k<float, POOL_MAX>), grid, block, 0, s, *d, idx, (const float*)dy, (float*)dx, CK, (unsigned)total);
    } else {
        if (d->dtype == SEG_BF16)
            hipLaunchKernelGGL((pool_bwd_k<bf16, POOL_AVG>), grid, block, 0, s, *d, idx, (const bf16*)dy, (bf16*)dx, CK, (unsigned)total);
        else if (d->dtype == SEG_F16)
            hipLaunchKernelGGL((pool_bwd_k<f16, POOL_AVG>), grid, block, 0, s, *d, idx, (const f16*)dy, (f16*)dx, CK, (unsigned)total);
        else
            hipLaunchKernelGGL((pool_bwd_k<float, POOL_AVG>), grid, block, 0, s, *d, idx, (const float*)dy, (float*)dx, CK, (unsigned)total);
    }
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

// Shared launch of the pad and the crop: y [N, YH, YW] from x [N, XH, XW].
static int shift_copy(const void* x, int ldx, int XH, int XW, void* y, int ldy, int YH, int YW, int N, int C, int top,
                      int left, int dtype, void* stream) {
    if (!x || !y || !dtype_ok(dtype) || !aligned16(x) || !aligned16(y)) return SEG_EINVAL;
    if (N < 1 || XH < 1 || XW < 1 || YH < 1 || YW < 1 || C < 1) return SEG_EINVAL;
    const int epc = epc_of(dtype);
    if (C % epc || ldx % epc || ldy % epc || ldx < C || ldy < C) return SEG_EINVAL;
    if ((long)N * XH * XW * ldx >= LIMIT || (long)N * YH * YW * ldy >= LIMIT) return SEG_EINVAL;
    const unsigned CK = (unsigned)(C / epc);
    const long total = (long)N * YH * YW * CK;
    const dim3 grid(seg_grid_1d(total, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SEG_BF16)
        hipLaunchKernelGGL(shift_copy_k<bf16>, grid, block, 0, s, (const bf16*)x, ldx, XH, XW, (bf16*)y, ldy, (unsigned)YH, (unsigned)YW, top, left, CK, (unsigned)total);
    else if (dtype == SEG_F16)
        hipLaunchKernelGGL(shift_copy_k<f16>, grid, block, 0, s, (const f16*)x, ldx, XH, XW, (f16*)y, ldy, (unsigned)YH, (unsigned)YW, top, left, CK, (unsigned)total);
    else
        hipLaunchKernelGGL(shift_copy_k<float>, grid, block, 0, s, (const float*)x, ldx, XH, XW, (float*)y, ldy, (unsigned)YH, (unsigned)YW, top, left, CK, (unsigned)total);
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

static bool pads_ok(int H, int W, int top, int bottom, int left, int right) {
    if (top < 0 || bottom < 0 || left < 0 || right < 0) return false;
    return (long)H + top + bottom < LIMIT && (long)W + left + right < LIMIT;
}

extern "C" int seg_pad2d_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int top, int bottom,
                             int left, int right, int dtype, void* stream) {
    if (H < 1 || W < 1 || !pads_ok(H, W, top, bottom, left, right)) return SEG_EINVAL;
    return shift_copy(x, ldx, H, W, y, ldy, H + top + bottom, W + left + right, N, C, top, left, dtype, stream);
}

extern "C" int seg_pad2d_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C, int top,
                             int bottom, int left, int right, int dtype, void* stream) {
    if (H < 1 || W < 1 || !pads_ok(H, W, top, bottom, left, right)) return SEG_EINVAL;
    return shift_copy(dy, lddy, H + top + bottom, W + left + right, dx, lddx, H, W, N, C, -top, -left, dtype, stream);
}
