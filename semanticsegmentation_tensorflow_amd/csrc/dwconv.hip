// tf.nn.depthwise_conv2d with channel multiplier 1 (SepConv_BN:
// Network/model/EfficientNet.py:426-462, DeepLabv3Plus.py:23-58): forward,
// input gradient and filter gradient.  One filter per channel is about 2 R S
// FLOP per element against 4 bytes moved in bf16, so these are HBM-bound VALU
// kernels: 16-byte chunks per lane, vector loads and stores only, fp32
// accumulation rounded once, the fp32 master filter [R, S, c_valid] read as it
// is.  Every load is guarded by the source extent and every store by the
// destination extent, so a tap that falls in the padding costs a compare.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ uint4 ldc(const T* p) { return *reinterpret_cast<const uint4*>(p); }
template <typename T>
__device__ __forceinline__ void stc(T* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }

constexpr int TW = 4;           // destination pixels along W per lane
constexpr int NT = 9;           // taps per filter-gradient workgroup
constexpr int WG_PIX = 128;     // pixels per filter-gradient partial row, at least
constexpr int WG_ROWS = 512;    // partial rows, at most

// Source coordinate along one axis of tap t for destination coordinate o, or
// -1.  Forward: o * s - pad + t * dil inside [0, n).  Input gradient: the
// output o' with o' * s - pad + t * dil == o, where there is one.
template <bool BWD>
__device__ __forceinline__ int src_coord(int o, int t, int s, int pad, int dil, int n) {
    if constexpr (!BWD) {
        const int i = o * s - pad + t * dil;
        return (i >= 0 && i < n) ? i : -1;
    } else {
        const int u = o + pad - t * dil;
        if (u < 0) return -1;
        const int i = u / s;
        return (i * s == u && i < n) ? i : -1;
    }
}

// 3 x 3 at stride 1, any dilation (every SepConv_BN of the models): forward and
// input gradient.  At stride 1 both are a 3 x 3 window over the source grid,
// dst[h, w] = sum_k src[h + off_h + kr dil_h, w + off_w + kq dil_w] tw[kr, kq]
// (the gradient with the taps reversed), and a dilated window only ever joins
// pixels of one phase (h mod dil_h, w mod dil_w).  So a lane owns one chunk of
// TW destination pixels dil_w apart -- their TW + 2 source columns serve all
// 3 TW products of a window row -- and walks RL destination rows dil_h apart:
// every source row is loaded once per walk and added into the three outputs
// whose window holds it, RL + 2 rows of TW + 2 loads for RL * TW outputs.  The
// nine filter chunks and three rows of accumulators stay in registers.
constexpr int RL = 4;
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void dw_rows3_k(seg_dwconv_desc d, const T* __restrict__ src,
                                                  const float* __restrict__ w, T* __restrict__ dst, int CK, int WSP,
                                                  int PW, int PH, int SEGS, int items) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int gx = blockIdx.x * 256 + threadIdx.x;
    if (gx >= CK * WSP * PW) return;                      // PW, PH: the phases that hold a destination pixel
    const int cc = gx % CK, t0 = gx / CK;
    const int strip = t0 % WSP, b = t0 / WSP;             // b: the column phase
    const int SH = BWD ? d.OH : d.H, SW = BWD ? d.OW : d.W, lds = BWD ? d.ldy : d.ldx;
    const int DH = BWD ? d.H : d.OH, DW = BWD ? d.W : d.OW, ldd = BWD ? d.ldx : d.ldy;
    const int c0 = cc * EPC;
    const int offh = BWD ? d.pad_top - 2 * d.dil_h : -d.pad_top;
    const int wd0 = b + strip * TW * d.dil_w;             // destination column of j = 0
    const int ws0 = wd0 + (BWD ? d.pad_left - 2 * d.dil_w : -d.pad_left);   // source column of m = 0

    float tw[9][EPC];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < EPC; ++e) tw[t][e] = c0 + e < d.c_valid ? w[(BWD ? 8 - t : t) * d.c_valid + c0 + e] : 0.f;

    for (int item = blockIdx.y; item < items; item += gridDim.y) {
        const int seg = item % SEGS, t1 = item / SEGS;
        const int a = t1 % PH, n = t1 / PH;               // a: the row phase
        const int i0 = seg * RL;                          // first output of the walk, in rows of the phase
        float acc[3][TW][EPC];
#pragma unroll
        for (int u = 0; u < RL + 2; ++u) {
            // step u: source row i0 + u of the phase is row kr of output i0 + u - kr
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[u % 3][j][e] = 0.f;
            const int sr = a + offh + (i0 + u) * d.dil_h;
            if (sr >= 0 && sr < SH) {
                const T* srow = src + ((long)n * SH + sr) * SW * lds + c0;
                uint4 raw[TW + 2];
#pragma unroll
                for (int m = 0; m < TW + 2; ++m) {
                    const int c = ws0 + m * d.dil_w;
                    raw[m] = make_uint4(0u, 0u, 0u, 0u);
                    if (c >= 0 && c < SW) raw[m] = ldc(srow + (long)c * lds);
                }
#pragma unroll
                for (int m = 0; m < TW + 2; ++m) {
                    float v[EPC];
                    Chunk<T>::unpack(raw[m], v);
#pragma unroll
                    for (int kr = 0; kr < 3; ++kr) {
                        if (u - kr < 0 || u - kr >= RL) continue;
#pragma unroll
                        for (int kq = 0; kq < 3; ++kq) {
                            const int j = m - kq;
                            if (j < 0 || j >= TW) continue;
#pragma unroll
                            for (int e = 0; e < EPC; ++e)
                                acc[(u - kr) % 3][j][e] = fmaf(v[e], tw[kr * 3 + kq][e], acc[(u - kr) % 3][j][e]);
                        }
                    }
                }
            }
            if (u >= 2) {                                 // output i0 + u - 2 has its three rows
                const int h = a + (i0 + u - 2) * d.dil_h;
                if (h < DH) {
                    T* drow = dst + ((long)n * DH + h) * DW * ldd + c0;
#pragma unroll
                    for (int j = 0; j < TW; ++j) {
                        const int c = wd0 + j * d.dil_w;
                        if (c >= DW) break;
#pragma unroll
                        for (int e = 0; e < EPC; ++e)
                            if (c0 + e >= d.c_valid) acc[(u - 2) % 3][j][e] = 0.f;
                        stc(drow + (long)c * ldd, Chunk<T>::pack(acc[(u - 2) % 3][j]));
                    }
                }
            }
        }
    }
}

// The general form (any filter up to 7 x 7, any stride): forward (BWD = false:
// src x, dst y) and input gradient (BWD = true: src dy, dst dx; a gather, dst
// overwritten).  A lane owns one chunk of TW destination pixels along W and
// walks the destination rows blockIdx.y, + gridDim.y, ...; one guarded load
// per (destination pixel, tap).  With KR x KS known (3 x 3) the taps stay in
// registers for the whole walk; otherwise each tap's filter chunk comes from
// the (cached) master filter.
template <typename T, int KR, int KS, bool BWD>
__global__ __launch_bounds__(256) void dw_gather_k(seg_dwconv_desc d, const T* __restrict__ src,
                                                   const float* __restrict__ w, T* __restrict__ dst, int CK, int WS,
                                                   int rows) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int gx = blockIdx.x * 256 + threadIdx.x;
    if (gx >= CK * WS) return;
    const int cc = gx % CK, w0 = (gx / CK) * TW;
    const int SH = BWD ? d.OH : d.H, SW = BWD ? d.OW : d.W, lds = BWD ? d.ldy : d.ldx;
    const int DH = BWD ? d.H : d.OH, DW = BWD ? d.W : d.OW, ldd = BWD ? d.ldx : d.ldy;
    const int RR = KR > 0 ? KR : d.R, SS = KS > 0 ? KS : d.S;
    const int c0 = cc * EPC;

    float taps[KR > 0 ? KR * KS : 1][EPC];
    if constexpr (KR > 0) {
#pragma unroll
        for (int t = 0; t < KR * KS; ++t)
#pragma unroll
            for (int e = 0; e < EPC; ++e) taps[t][e] = c0 + e < d.c_valid ? w[t * d.c_valid + c0 + e] : 0.f;
    }

    for (int row = blockIdx.y; row < rows; row += gridDim.y) {
        const int n = row / DH, h = row - n * DH;
        float acc[TW][EPC];
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[j][e] = 0.f;
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int ih = src_coord<BWD>(h, r, d.stride, d.pad_top, d.dil_h, SH);
            if (ih < 0) continue;
            const T* srow = src + ((long)n * SH + ih) * SW * lds + c0;
#pragma unroll
            for (int q = 0; q < SS; ++q) {
                float wv[EPC];
                if constexpr (KR > 0) {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) wv[e] = taps[r * KS + q][e];
                } else {
                    const float* wp = w + (long)(r * SS + q) * d.c_valid + c0;
#pragma unroll
                    for (int e = 0; e < EPC; ++e) wv[e] = c0 + e < d.c_valid ? wp[e] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    const int iw = w0 + j < DW ? src_coord<BWD>(w0 + j, q, d.stride, d.pad_left, d.dil_w, SW) : -1;
                    if (iw < 0) continue;
                    float v[EPC];
                    Chunk<T>::unpack(ldc(srow + (long)iw * lds), v);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[j][e] = fmaf(v[e], wv[e], acc[j][e]);
                }
            }
        }
        T* drow = dst + ((long)row * DW + w0) * ldd + c0;
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            if (w0 + j >= DW) break;
#pragma unroll
            for (int e = 0; e < EPC; ++e)
                if (c0 + e >= d.c_valid) acc[j][e] = 0.f;     // padding channels: exact zeros
            stc(drow + (long)j * ldd, Chunk<T>::pack(acc[j]));
        }
    }
}

// Filter gradient, first pass.  Workgroup (blockIdx.x: LPP chunks) x
// (blockIdx.y: a pixel range of `per` outputs) x (blockIdx.z: NT taps); the 256
// / LPP row lanes of a chunk stride the range, each lane summing its NT taps
// in registers, then the row lanes are added in lane order through LDS and
// written as one fp32 partial row part[blockIdx.y][R * S][C].
template <typename T>
__global__ __launch_bounds__(256) void dw_wgrad_k(seg_dwconv_desc d, const T* __restrict__ x,
                                                  const T* __restrict__ dy, float* __restrict__ part, int CK, int LPP,
                                                  int P, int per) {
    constexpr int EPC = dt_traits<T>::EPC;
    __shared__ __attribute__((aligned(16))) float red[256 * EPC];
    const int RS = d.R * d.S;
    const int cl = threadIdx.x % LPP, rl = threadIdx.x / LPP, RL = 256 / LPP;
    const int chunk = blockIdx.x * LPP + cl;
    const bool live = chunk < CK;
    const int t0 = blockIdx.z * NT;
    const int p0 = blockIdx.y * per, p1 = min(P, p0 + per);
    float acc[NT][EPC];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[k][e] = 0.f;
    if (live) {
        for (int pix = p0 + rl; pix < p1; pix += RL) {
            const int ow = pix % d.OW, t = pix / d.OW;
            const int oh = t % d.OH, n = t / d.OH;
            float g[EPC];
            Chunk<T>::unpack(ldc(dy + (long)pix * d.ldy + chunk * EPC), g);
            const T* xn = x + (long)n * d.H * d.W * d.ldx + chunk * EPC;
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int tap = t0 + k;
                if (tap >= RS) break;
                const int r = tap / d.S, q = tap - r * d.S;
                const int ih = oh * d.stride - d.pad_top + r * d.dil_h;
                const int iw = ow * d.stride - d.pad_left + q * d.dil_w;
                if (ih < 0 || ih >= d.H || iw < 0 || iw >= d.W) continue;
                float v[EPC];
                Chunk<T>::unpack(ldc(xn + ((long)ih * d.W + iw) * d.ldx), v);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[k][e] = fmaf(v[e], g[e], acc[k][e]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int tap = t0 + k;
        if (tap >= RS) break;                              // uniform over the workgroup
#pragma unroll
        for (int e = 0; e < EPC; e += 4)
            *reinterpret_cast<float4*>(&red[threadIdx.x * EPC + e]) =
                make_float4(acc[k][e], acc[k][e + 1], acc[k][e + 2], acc[k][e + 3]);
        __syncthreads();
        if (rl == 0 && live) {
            float o[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) o[e] = acc[k][e];
            for (int rr = 1; rr < RL; ++rr) {
#pragma unroll
                for (int e = 0; e < EPC; e += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(&red[(rr * LPP + cl) * EPC + e]);
                    o[e] += v.x; o[e + 1] += v.y; o[e + 2] += v.z; o[e + 3] += v.w;
                }
            }
            float* out = part + ((long)blockIdx.y * RS + tap) * d.C + chunk * EPC;
#pragma unroll
            for (int e = 0; e < EPC; e += 4)
                *reinterpret_cast<float4*>(out + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
        }
        __syncthreads();
    }
}

// Filter gradient, second pass: dw[tap][c] = the sum over the partial rows, in
// row order (8 columns x 32 row groups per workgroup, the form of the bias
// gradient's column sums); the padded channels of a row are dropped.
__global__ __launch_bounds__(256) void dw_wgrad_sum_k(const float* __restrict__ part, int nrows, int RS, int C,
                                                      int c_valid, float* __restrict__ dw) {
    __shared__ float s[32][9];
    const int cl = threadIdx.x & 7, rg = threadIdx.x >> 3;
    const int col = blockIdx.x * 8 + cl;
    const int tap = col / C, c = col - tap * C;
    const bool live = tap < RS && c < c_valid;
    float acc = 0.f;
    if (live)
        for (int r = rg; r < nrows; r += 32) acc += part[((long)r * RS + tap) * C + c];
    s[rg][cl] = acc;
    __syncthreads();
    if (threadIdx.x < 8 && live) {
        float t = 0.f;
        for (int r = 0; r < 32; ++r) t += s[r][cl];
        dw[(long)tap * c_valid + c] = t;
    }
}

inline int epc_of(int dtype) { return dtype == SEG_F32 ? 4 : 8; }
inline bool dtype_ok(int dtype) { return dtype == SEG_F32 || dtype == SEG_BF16 || dtype == SEG_F16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr long LIMIT = 1L << 31;

// TF's output size and leading pad along one axis on the effective window;
// false when there is no output.
bool axis_geom(int in, int k, int dil, int s, int padding, int* out, int* before) {
    const long k_eff = (long)(k - 1) * dil + 1;
    if (padding == 0) {
        *out = (in + s - 1) / s;
        const long total = (long)(*out - 1) * s + k_eff - in;
        *before = total > 0 ? (int)(total / 2) : 0;
    } else {
        if (in < k_eff) return false;
        *out = (int)((in - k_eff) / s + 1);
        *before = 0;
    }
    return *out >= 1;
}

// Everything a launch relies on, re-derived from the descriptor's own fields
// (a caller may have built or edited it by hand): SEG_OK or the refusal.
int desc_status(const seg_dwconv_desc* d) {
    if (!d || !dtype_ok(d->dtype)) return SEG_EINVAL;
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->C < 1 || d->c_valid < 1 || d->R < 1 || d->S < 1 || d->stride < 1 ||
        d->dil_h < 1 || d->dil_w < 1 || d->pad_top < 0 || d->pad_left < 0)
        return SEG_EINVAL;
    if (d->R > 7 || d->S > 7) return SEG_EINVAL;
    if (d->C % 8 || d->c_valid > d->C) return SEG_EALIGN;
    if (d->ldx % epc_of(d->dtype) || d->ldy % epc_of(d->dtype)) return SEG_EALIGN;
    if (d->ldx < d->C || d->ldy < d->C) return SEG_EINVAL;
    if (d->stride > 1 && (d->dil_h > 1 || d->dil_w > 1)) return SEG_ESHAPE;
    if (d->OH < 1 || d->OW < 1) return SEG_ESHAPE;
    if ((long)d->N * d->H * d->W * d->ldx >= LIMIT || (long)d->N * d->OH * d->OW * d->ldy >= LIMIT) return SEG_EINVAL;
    // the index math also forms (pad + tap * dilation) and (out * stride): keep them in int
    if ((long)d->pad_top + 6L * d->dil_h + d->H >= LIMIT || (long)d->pad_left + 6L * d->dil_w + d->W >= LIMIT ||
        (long)d->OH * d->stride >= LIMIT || (long)d->OW * d->stride >= LIMIT)
        return SEG_EINVAL;
    return SEG_OK;
}

int wgrad_rows(const seg_dwconv_desc* d) {
    const long P = (long)d->N * d->OH * d->OW;
    const long rows = (P + WG_PIX - 1) / WG_PIX;
    return (int)(rows < 1 ? 1 : rows > WG_ROWS ? WG_ROWS : rows);
}

template <typename T, bool BWD>
void launch_gather(const seg_dwconv_desc* d, const void* src, const float* w, void* dst, hipStream_t s) {
    const int CK = d->C / dt_traits<T>::EPC;
    const int DW = BWD ? d->W : d->OW, DH = BWD ? d->H : d->OH;
    const int WS = (DW + TW - 1) / TW;
    const int rows = d->N * DH;
    const int gx = (int)(((long)CK * WS + 255) / 256);
    const int cap = 2048 * 8 / gx;
    const dim3 grid(gx, rows < cap ? rows : (cap < 1 ? 1 : cap)), block(256);
    if (d->R == 3 && d->S == 3 && d->stride == 1) {
        const int PW = d->dil_w < DW ? d->dil_w : DW, PH = d->dil_h < DH ? d->dil_h : DH;
        const int WSP = ((DW + d->dil_w - 1) / d->dil_w + TW - 1) / TW;
        const int SEGS = ((DH + d->dil_h - 1) / d->dil_h + RL - 1) / RL;
        const int items = d->N * PH * SEGS;
        const int g3 = (int)(((long)CK * WSP * PW + 255) / 256);
        const int cap3 = 2048 * 8 / g3;
        const dim3 grid3(g3, items < cap3 ? items : (cap3 < 1 ? 1 : cap3));
        hipLaunchKernelGGL((dw_rows3_k<T, BWD>), grid3, block, 0, s, *d, (const T*)src, w, (T*)dst, CK, WSP, PW, PH, SEGS,
                           items);
    } else if (d->R == 3 && d->S == 3)
        hipLaunchKernelGGL((dw_gather_k<T, 3, 3, BWD>), grid, block, 0, s, *d, (const T*)src, w, (T*)dst, CK, WS, rows);
    else
        hipLaunchKernelGGL((dw_gather_k<T, 0, 0, BWD>), grid, block, 0, s, *d, (const T*)src, w, (T*)dst, CK, WS, rows);
}

template <bool BWD>
int gather(const seg_dwconv_desc* d, const void* src, const float* w, void* dst, void* stream) {
    const int st = desc_status(d);
    if (st != SEG_OK) return st;
    if (!src || !w || !dst || !aligned16(src) || !aligned16(dst) || ((uintptr_t)w & 3)) return SEG_EINVAL;
    // the grid's x extent: chunks x strips of one destination row
    if ((long)(d->C / epc_of(d->dtype)) * (((BWD ? d->W : d->OW) + TW - 1) / TW) >= LIMIT) return SEG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (d->dtype == SEG_BF16) launch_gather<bf16, BWD>(d, src, w, dst, s);
    else if (d->dtype == SEG_F16) launch_gather<f16, BWD>(d, src, w, dst, s);
    else launch_gather<float, BWD>(d, src, w, dst, s);
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

template <typename T>
void launch_wgrad(const seg_dwconv_desc* d, const void* x, const void* dy, float* part, int rows, hipStream_t s) {
    const int CK = d->C / dt_traits<T>::EPC;
    int LPP = 1;
    while (LPP < CK && LPP < 64) LPP *= 2;
    const int P = d->N * d->OH * d->OW;
    const int per = (P + rows - 1) / rows;
    const dim3 grid((CK + LPP - 1) / LPP, rows, (d->R * d->S + NT - 1) / NT), block(256);
    hipLaunchKernelGGL(dw_wgrad_k<T>, grid, block, 0, s, *d, (const T*)x, (const T*)dy, part, CK, LPP, P, per);
}

}  // namespace

extern "C" int seg_dwconv_desc_init(seg_dwconv_desc* d, int N, int H, int W, int C, int c_valid, int R, int S,
                                    int stride, int dil_h, int dil_w, int padding, int dtype) {
    if (!d || !dtype_ok(dtype) || (padding != 0 && padding != 1)) return SEG_EINVAL;
    seg_dwconv_desc t;
    t.N = N; t.H = H; t.W = W; t.C = C;
    t.R = R; t.S = S; t.stride = stride; t.dil_h = dil_h; t.dil_w = dil_w;
    t.OH = t.OW = 1; t.pad_top = t.pad_left = 0;
    t.ldx = C; t.ldy = C;
    t.c_valid = c_valid; t.dtype = dtype;
    int st = desc_status(&t);                 // sizes, alignment, TF's stride / dilation rule
    if (st != SEG_OK) return st;
    if (!axis_geom(H, R, dil_h, stride, padding, &t.OH, &t.pad_top) ||
        !axis_geom(W, S, dil_w, stride, padding, &t.OW, &t.pad_left))
        return SEG_ESHAPE;
    st = desc_status(&t);                     // element counts with the real output size
    if (st != SEG_OK) return st;
    *d = t;
    return SEG_OK;
}

extern "C" int seg_dwconv2d_fwd(const seg_dwconv_desc* d, const void* x, const float* w, void* y, void* stream) {
    return gather<false>(d, x, w, y, stream);
}

extern "C" int seg_dwconv2d_bwd_data(const seg_dwconv_desc* d, const void* dy, const float* w, void* dx,
                                     void* stream) {
    return gather<true>(d, dy, w, dx, stream);
}

extern "C" size_t seg_dwconv_bwd_filter_workspace(const seg_dwconv_desc* d) {
    if (desc_status(d) != SEG_OK) return 0;
    return (size_t)wgrad_rows(d) * d->R * d->S * d->C * sizeof(float);
}

extern "C" int seg_dwconv2d_bwd_filter(const seg_dwconv_desc* d, const void* x, const void* dy, float* dw, void* ws,
                                       size_t ws_bytes, void* stream) {
    const int st = desc_status(d);
    if (st != SEG_OK) return st;
    if (!x || !dy || !dw || !ws || !aligned16(x) || !aligned16(dy) || !aligned16(ws) || ((uintptr_t)dw & 3))
        return SEG_EINVAL;
    if (ws_bytes < seg_dwconv_bwd_filter_workspace(d)) return SEG_EWORKSPACE;
    const int rows = wgrad_rows(d), RS = d->R * d->S;
    float* part = (float*)ws;
    hipStream_t s = (hipStream_t)stream;
    if (d->dtype == SEG_BF16) launch_wgrad<bf16>(d, x, dy, part, rows, s);
    else if (d->dtype == SEG_F16) launch_wgrad<f16>(d, x, dy, part, rows, s);
    else launch_wgrad<float>(d, x, dy, part, rows, s);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(dw_wgrad_sum_k, dim3((RS * d->C + 7) / 8), dim3(256), 0, s, part, rows, RS, d->C, d->c_valid,
                       dw);
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}
