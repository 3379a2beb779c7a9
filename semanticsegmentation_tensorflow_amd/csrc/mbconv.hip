// The pieces of MBConvBlock (Network/model/EfficientNet.py:153-210) that are not
// a convolution: frozen-stat BatchNorm + swish / sigmoid (forward and gradient),
// the squeeze (a spatial mean of any width), and the excite multiply x * s[n, c]
// (forward and gradient).  All of them move 2-6 bytes per element for a handful
// of FLOP: HBM-bound VALU kernels on NHWC with pixel strides, 16-byte chunks per
// lane, fp32 arithmetic rounded once, vector loads and stores only.
//
// One geometry for all: the C / EPC chunks of a pixel are cut into `groups`
// chunk groups of LPP chunks (blockIdx.x); the 256 lanes of a workgroup are
// rows x LPP, a lane keeps its chunk -- so its per-channel operands (the affine,
// the gate s[n, c]) are loaded once -- and walks pixels rows apart.  Reductions
// are two passes without float atomics: every workgroup adds its row lanes in
// row order through LDS and writes one fp32 partial row, and a second kernel
// sums the partial rows in a fixed order (bn_finish_k's 8 channels x 32 row
// groups).  Bit-identical from run to run.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ uint4 ldc(const T* p) { return *reinterpret_cast<const uint4*>(p); }
template <typename T>
__device__ __forceinline__ void stc(T* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }

constexpr long LIMIT = 1L << 31;
constexpr int BN_ROWS_MAX = 512;    // partial rows of the BatchNorm gradient, at most
constexpr int BN_ROW_ELEMS = 8192;  // elements per partial row, at least (a few sweeps of a workgroup)
constexpr int SE_SLICES_MAX = 128;  // pixel slices per image of the squeeze / excite sums, at most
constexpr int SE_SLICE_PIX = 128;   // pixels per slice, at least

struct Geom {
    int CK, LPP, rows, groups;
};

// groups in 1..8 with the most live lanes: CK * rows of groups * 256
Geom geom_of(int C, int epc) {
    Geom g, best;
    g.CK = C / epc;
    best = g;
    long best_num = -1, best_den = 1;
    for (int n = 1; n <= 8; ++n) {
        g.groups = n;
        g.LPP = (g.CK + n - 1) / n;
        if (g.LPP > 256) continue;
        g.rows = 256 / g.LPP;
        const long num = (long)g.CK * g.rows, den = (long)n * 256;
        if (best_num < 0 || num * best_den > best_num * den) {
            best = g;
            best_num = num;
            best_den = den;
        }
    }
    if (best_num < 0) {                     // more than 2048 chunks: 256 per group
        best.LPP = 256;
        best.rows = 1;
        best.groups = (best.CK + 255) / 256;
    }
    return best;
}

// sigmoid(z) = 1 / (1 + exp(-z)): exp overflows to inf for z < -88.7 and the
// quotient is then 0; for large z exp(-z) underflows to 0 and the quotient is 1
__device__ __forceinline__ float sigmoid_f(float z) { return 1.0f / (1.0f + expf(-z)); }

// y = act(x * scale + shift); AFFINE false: scale 1, shift 0
template <typename T, bool AFFINE>
__global__ __launch_bounds__(256) void bn_act_fwd_k(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float inv, int P, int cv, int act, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    float sc[EPC], sh[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const bool ok = c0 + e < cv;
        sc[e] = AFFINE ? (ok ? gamma[c0 + e] * inv : 0.f) : 1.f;
        sh[e] = AFFINE ? (ok ? beta[c0 + e] : 0.f) : 0.f;
    }
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
        float v[EPC];
        Chunk<T>::unpack(ldc(x + (long)pix * ldx + c0), v);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float z = __builtin_fmaf(v[e], sc[e], sh[e]);
            const float s = sigmoid_f(z);
            const float o = act == SEG_ACT_SWISH ? z * s : s;
            v[e] = c0 + e < cv ? o : 0.f;                 // padding channels: exact zeros (sigmoid(0) is 0.5)
        }
        stc(y + (long)pix * ldy + c0, Chunk<T>::pack(v));
    }
}

// dz = dy * act'(z) recomputed from x; dx (+)= dz * scale; AFFINE: the lane's
// sums of dz * x and dz, the row lanes added in row order, one partial row
// part[blockIdx.y][2][C] per workgroup row
template <typename T, bool AFFINE>
__global__ __launch_bounds__(256) void bn_act_bwd_k(const T* __restrict__ x, int ldx, const T* __restrict__ dy,
                                                    int lddy, T* __restrict__ dx, int lddx,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float inv, float* __restrict__ part, int P, int C, int cv, int act,
                                                    int accumulate, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    __shared__ __attribute__((aligned(16))) float red[AFFINE ? 256 * EPC : 4];
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    const bool live = prow < g.rows && chunk < g.CK;
    const int c0 = chunk * EPC;
    float sc[EPC], sh[EPC], sg[EPC], sb[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const bool ok = live && c0 + e < cv;
        sc[e] = AFFINE ? (ok ? gamma[c0 + e] * inv : 0.f) : 1.f;
        sh[e] = AFFINE ? (ok ? beta[c0 + e] : 0.f) : 0.f;
        sg[e] = sb[e] = 0.f;
    }
    if (live) {
        const int step = gridDim.y * g.rows;
        for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
            float xv[EPC], d[EPC], old[EPC];
            Chunk<T>::unpack(ldc(x + (long)pix * ldx + c0), xv);
            Chunk<T>::unpack(ldc(dy + (long)pix * lddy + c0), d);
            if (accumulate) Chunk<T>::unpack(ldc(dx + (long)pix * lddx + c0), old);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float z = __builtin_fmaf(xv[e], sc[e], sh[e]);
                const float s = sigmoid_f(z);
                const float t = 1.0f - s;
                const float gz = act == SEG_ACT_SWISH ? s * (1.0f + z * t) : s * t;
                const float dz = c0 + e < cv ? d[e] * gz : 0.f;
                if (AFFINE) {
                    sb[e] += dz;
                    sg[e] = __builtin_fmaf(dz, xv[e], sg[e]);
                }
                d[e] = dz * sc[e];
                if (accumulate) d[e] += old[e];
            }
            stc(dx + (long)pix * lddx + c0, Chunk<T>::pack(d));
        }
    }
    if constexpr (AFFINE) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int e = 0; e < EPC; e += 4)
                *reinterpret_cast<float4*>(&red[threadIdx.x * EPC + e]) =
                    k == 0 ? make_float4(sg[e], sg[e + 1], sg[e + 2], sg[e + 3])
                           : make_float4(sb[e], sb[e + 1], sb[e + 2], sb[e + 3]);
            __syncthreads();
            if (prow == 0 && live) {
                float o[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) o[e] = k == 0 ? sg[e] : sb[e];
                for (int rr = 1; rr < g.rows; ++rr) {
#pragma unroll
                    for (int e = 0; e < EPC; e += 4) {
                        const float4 v = *reinterpret_cast<const float4*>(&red[(rr * g.LPP + cl) * EPC + e]);
                        o[e] += v.x; o[e + 1] += v.y; o[e + 2] += v.z; o[e + 3] += v.w;
                    }
                }
                float* out = part + ((long)blockIdx.y * 2 + k) * C + c0;
#pragma unroll
                for (int e = 0; e < EPC; e += 4)
                    *reinterpret_cast<float4*>(out + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
            }
            __syncthreads();
        }
    }
}

// dgamma / dbeta from the partial rows in row order (bn_finish_k's form: 8
// channels x 32 row groups per workgroup)
__global__ __launch_bounds__(256) void bn_act_finish_k(const float* __restrict__ part, int nrows, int C, int cv,
                                                       float inv, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta) {
    __shared__ float sg[32][9], sb[32][9];
    const int cl = threadIdx.x & 7, rg = threadIdx.x >> 3;
    const int k = blockIdx.x * 8 + cl;
    float a = 0.f, b = 0.f;
    if (k < cv)
        for (int r = rg; r < nrows; r += 32) {
            a += part[((long)r * 2) * C + k];
            b += part[((long)r * 2 + 1) * C + k];
        }
    sg[rg][cl] = a;
    sb[rg][cl] = b;
    __syncthreads();
    if (threadIdx.x < 8 && k < cv) {
        float ta = 0.f, tb = 0.f;
        for (int r = 0; r < 32; ++r) {
            ta += sg[r][cl];
            tb += sb[r][cl];
        }
        dgamma[k] = ta * inv;
        dbeta[k] = tb;
    }
}

// The spatial sums of the squeeze (MODE 0: of x), and the excite gradient
// (MODE 1: dx (+)= dy * s written on the way, the sum of dy * x).  Workgroup
// (chunk group) x (pixel slice) x (image): never two images in one workgroup.
// part[n][slice][C].
template <typename T, int MODE>
__global__ __launch_bounds__(256) void se_sum_k(const T* __restrict__ x, int ldx, const T* __restrict__ s,
                                                const T* __restrict__ dy, int lddy, T* __restrict__ dx, int lddx,
                                                float* __restrict__ part, int HW, int C, int cv, int per,
                                                int accumulate, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    __shared__ __attribute__((aligned(16))) float red[256 * EPC];
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    const bool live = prow < g.rows && chunk < g.CK;
    const int c0 = chunk * EPC;
    const int n = blockIdx.z;
    const int p0 = blockIdx.y * per, p1 = min(HW, p0 + per);
    float acc[EPC], sv[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = sv[e] = 0.f;
    if (live) {
        if constexpr (MODE == 1) Chunk<T>::unpack(ldc(s + (long)n * C + c0), sv);
        for (int pix = p0 + prow; pix < p1; pix += g.rows) {
            const long q = (long)n * HW + pix;
            float v[EPC];
            Chunk<T>::unpack(ldc(x + q * ldx + c0), v);
            if constexpr (MODE == 0) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += v[e];
            } else {
                float d[EPC], old[EPC];
                Chunk<T>::unpack(ldc(dy + q * lddy + c0), d);
                if (accumulate) Chunk<T>::unpack(ldc(dx + q * lddx + c0), old);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const bool ok = c0 + e < cv;
                    acc[e] = __builtin_fmaf(ok ? d[e] : 0.f, v[e], acc[e]);
                    float o = ok ? d[e] * sv[e] : 0.f;
                    if (accumulate) o += old[e];
                    d[e] = o;
                }
                stc(dx + q * lddx + c0, Chunk<T>::pack(d));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPC; e += 4)
        *reinterpret_cast<float4*>(&red[threadIdx.x * EPC + e]) =
            make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
    __syncthreads();
    if (prow == 0 && live) {
        for (int rr = 1; rr < g.rows; ++rr) {
#pragma unroll
            for (int e = 0; e < EPC; e += 4) {
                const float4 v = *reinterpret_cast<const float4*>(&red[(rr * g.LPP + cl) * EPC + e]);
                acc[e] += v.x; acc[e + 1] += v.y; acc[e + 2] += v.z; acc[e + 3] += v.w;
            }
        }
        float* out = part + ((long)n * gridDim.y + blockIdx.y) * C + c0;
#pragma unroll
        for (int e = 0; e < EPC; e += 4)
            *reinterpret_cast<float4*>(out + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
    }
}

// y[n, c] = scale * (the slices of part[n], summed in a fixed order: 8 channels
// x 32 slice groups per workgroup, bn_finish_k's form), rounded once; padding
// channels get zeros
template <typename T>
__global__ __launch_bounds__(256) void se_finish_k(const float* __restrict__ part, int slices, int C, int cv,
                                                   float scale, T* __restrict__ y) {
    __shared__ float sm[32][9];
    const int cl = threadIdx.x & 7, rg = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl, n = blockIdx.y;
    float a = 0.f;
    if (c < cv)
        for (int r = rg; r < slices; r += 32) a += part[((long)n * slices + r) * C + c];
    sm[rg][cl] = a;
    __syncthreads();
    if (threadIdx.x < 8) {                     // C % 8 == 0: c < C
        float t = 0.f;
        for (int r = 0; r < 32; ++r) t += sm[r][cl];
        y[(long)n * C + c] = from_f32<T>(c < cv ? t * scale : 0.f);
    }
}

// y = x * s[n, c]
template <typename T>
__global__ __launch_bounds__(256) void se_excite_fwd_k(const T* __restrict__ x, int ldx, const T* __restrict__ s,
                                                       T* __restrict__ y, int ldy, int HW, int C, int cv, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    const int n = blockIdx.z;
    float sv[EPC];
    Chunk<T>::unpack(ldc(s + (long)n * C + c0), sv);
#pragma unroll
    for (int e = 0; e < EPC; ++e)
        if (c0 + e >= cv) sv[e] = 0.f;
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < HW; pix += step) {
        const long q = (long)n * HW + pix;
        float v[EPC];
        Chunk<T>::unpack(ldc(x + q * ldx + c0), v);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = c0 + e < cv ? v[e] * sv[e] : 0.f;
        stc(y + q * ldy + c0, Chunk<T>::pack(v));
    }
}

inline int epc_of(int dtype) { return dtype == SEG_F32 ? 4 : 8; }
inline bool dtype_ok(int dtype) { return dtype == SEG_F32 || dtype == SEG_BF16 || dtype == SEG_F16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// a [P, C] view with pixel stride ld: SEG_OK or the refusal
int view_status(const void* p, long P, int ld, int C, int dtype) {
    if (!p || !aligned16(p)) return SEG_EINVAL;
    if (ld % epc_of(dtype)) return SEG_EALIGN;
    if (ld < C) return SEG_EINVAL;
    if (P * (long)ld >= LIMIT) return SEG_EINVAL;
    return SEG_OK;
}

int chan_status(long P, int C, int cv, int dtype) {
    if (!dtype_ok(dtype) || P < 1 || C < 1 || cv < 1) return SEG_EINVAL;
    if (C % 8 || cv > C) return SEG_EALIGN;
    if (P >= LIMIT) return SEG_EINVAL;
    return SEG_OK;
}

int bn_rows(long P, int C) {
    const long r = (P * C + BN_ROW_ELEMS - 1) / BN_ROW_ELEMS;
    return (int)(r < 1 ? 1 : r > BN_ROWS_MAX ? BN_ROWS_MAX : r);
}

int se_slices(long HW) {
    const long r = (HW + SE_SLICE_PIX - 1) / SE_SLICE_PIX;
    return (int)(r < 1 ? 1 : r > SE_SLICES_MAX ? SE_SLICES_MAX : r);
}

// pixel rows of the grid for a plain (no partial rows) pass
int walk_rows(long P, const Geom& g) {
    const long r = (P + g.rows - 1) / g.rows;
    const long cap = std::max(1, 8192 / g.groups);
    return (int)(r < 1 ? 1 : r > cap ? cap : r);
}

int se_status(int N, int H, int W, int C, int cv, int dtype, long* HW) {
    if (N < 1 || H < 1 || W < 1 || N > 65535) return SEG_EINVAL;
    *HW = (long)H * W;
    return chan_status((long)N * *HW, C, cv, dtype);
}

#define MB_DISPATCH(dtype, ...)                               \
    do {                                                      \
        if ((dtype) == SEG_BF16) { using T = bf16; __VA_ARGS__; } \
        else if ((dtype) == SEG_F16) { using T = f16; __VA_ARGS__; } \
        else { using T = float; __VA_ARGS__; }               \
    } while (0)

}  // namespace

extern "C" int seg_bn_act_fwd(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta,
                              float eps, long P, int C, int c_valid, int act, int dtype, void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((st = view_status(x, P, ldx, C, dtype)) != SEG_OK || (st = view_status(y, P, ldy, C, dtype)) != SEG_OK)
        return st;
    if ((act != SEG_ACT_SWISH && act != SEG_ACT_SIGMOID) || !(eps >= 0.f)) return SEG_EINVAL;
    if ((gamma == nullptr) != (beta == nullptr) || ((uintptr_t)gamma & 3) || ((uintptr_t)beta & 3)) return SEG_EINVAL;
    const float inv = 1.0f / sqrtf(1.0f + eps);
    const Geom g = geom_of(C, epc_of(dtype));
    const dim3 grid(g.groups, walk_rows(P, g)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (gamma)
        MB_DISPATCH(dtype, hipLaunchKernelGGL((bn_act_fwd_k<T, true>), grid, block, 0, s, (const T*)x, ldx, (T*)y, ldy,
                                              gamma, beta, inv, (int)P, c_valid, act, g));
    else
        MB_DISPATCH(dtype, hipLaunchKernelGGL((bn_act_fwd_k<T, false>), grid, block, 0, s, (const T*)x, ldx, (T*)y,
                                              ldy, gamma, beta, inv, (int)P, c_valid, act, g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" size_t seg_bn_act_bwd_workspace(long P, int C) {
    if (P < 1 || C < 1 || C % 8 || P >= LIMIT) return 0;
    return (size_t)bn_rows(P, C) * 2 * C * sizeof(float);
}

extern "C" int seg_bn_act_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx,
                              const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, long P,
                              int C, int c_valid, int act, int flags, int dtype, void* ws, size_t ws_bytes,
                              void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((st = view_status(x, P, ldx, C, dtype)) != SEG_OK || (st = view_status(dy, P, lddy, C, dtype)) != SEG_OK ||
        (st = view_status(dx, P, lddx, C, dtype)) != SEG_OK)
        return st;
    if ((act != SEG_ACT_SWISH && act != SEG_ACT_SIGMOID) || !(eps >= 0.f) || (flags & ~2)) return SEG_EINVAL;
    if ((gamma == nullptr) != (beta == nullptr) || ((uintptr_t)gamma & 3) || ((uintptr_t)beta & 3)) return SEG_EINVAL;
    if (gamma && (!dgamma || !dbeta || ((uintptr_t)dgamma & 3) || ((uintptr_t)dbeta & 3))) return SEG_EINVAL;
    if (!gamma && (dgamma || dbeta)) return SEG_EINVAL;
    const float inv = 1.0f / sqrtf(1.0f + eps);
    const Geom g = geom_of(C, epc_of(dtype));
    const int acc = (flags & 2) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    if (!gamma) {
        const dim3 grid(g.groups, walk_rows(P, g)), block(256);
        MB_DISPATCH(dtype, hipLaunchKernelGGL((bn_act_bwd_k<T, false>), grid, block, 0, s, (const T*)x, ldx,
                                              (const T*)dy, lddy, (T*)dx, lddx, gamma, beta, inv, (float*)nullptr,
                                              (int)P, C, c_valid, act, acc, g));
        SEG_CHECK_LAUNCH();
        return SEG_OK;
    }
    if (!ws || !aligned16(ws)) return SEG_EINVAL;
    if (ws_bytes < seg_bn_act_bwd_workspace(P, C)) return SEG_EWORKSPACE;
    const int rows = bn_rows(P, C);
    const dim3 grid(g.groups, rows), block(256);
    MB_DISPATCH(dtype, hipLaunchKernelGGL((bn_act_bwd_k<T, true>), grid, block, 0, s, (const T*)x, ldx, (const T*)dy,
                                          lddy, (T*)dx, lddx, gamma, beta, inv, (float*)ws, (int)P, C, c_valid, act,
                                          acc, g));
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_act_finish_k, dim3((c_valid + 7) / 8), dim3(256), 0, s, (const float*)ws, rows, C, c_valid,
                       inv, dgamma, dbeta);
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" size_t seg_se_squeeze_workspace(int N, int H, int W, int C) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || C % 8) return 0;
    return (size_t)N * se_slices((long)H * W) * C * sizeof(float);
}

extern "C" int seg_se_squeeze(const void* x, int ldx, void* y, int N, int H, int W, int C, int c_valid, float scale,
                              void* ws, size_t ws_bytes, int dtype, void* stream) {
    long HW;
    int st = se_status(N, H, W, C, c_valid, dtype, &HW);
    if (st != SEG_OK) return st;
    if ((st = view_status(x, (long)N * HW, ldx, C, dtype)) != SEG_OK) return st;
    if (!y || !aligned16(y) || !ws || !aligned16(ws)) return SEG_EINVAL;
    if (ws_bytes < seg_se_squeeze_workspace(N, H, W, C)) return SEG_EWORKSPACE;
    const Geom g = geom_of(C, epc_of(dtype));
    const int slices = se_slices(HW);
    const int per = (int)((HW + slices - 1) / slices);
    const dim3 grid(g.groups, slices, N), block(256);
    hipStream_t s = (hipStream_t)stream;
    MB_DISPATCH(dtype, hipLaunchKernelGGL((se_sum_k<T, 0>), grid, block, 0, s, (const T*)x, ldx, (const T*)nullptr,
                                          (const T*)nullptr, 0, (T*)nullptr, 0, (float*)ws, (int)HW, C, c_valid, per,
                                          0, g));
    SEG_CHECK_LAUNCH();
    MB_DISPATCH(dtype, hipLaunchKernelGGL(se_finish_k<T>, dim3(C / 8, N), dim3(256), 0, s,
                                          (const float*)ws, slices, C, c_valid, scale, (T*)y));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" int seg_se_excite_fwd(const void* x, int ldx, const void* s_, void* y, int ldy, int N, int H, int W, int C,
                                 int c_valid, int dtype, void* stream) {
    long HW;
    int st = se_status(N, H, W, C, c_valid, dtype, &HW);
    if (st != SEG_OK) return st;
    if ((st = view_status(x, (long)N * HW, ldx, C, dtype)) != SEG_OK ||
        (st = view_status(y, (long)N * HW, ldy, C, dtype)) != SEG_OK)
        return st;
    if (!s_ || !aligned16(s_)) return SEG_EINVAL;
    const Geom g = geom_of(C, epc_of(dtype));
    const long per_n = std::max(1L, 8192L / ((long)g.groups * N));
    const long r = (HW + g.rows - 1) / g.rows;
    const dim3 grid(g.groups, (unsigned)(r < per_n ? r : per_n), N), block(256);
    MB_DISPATCH(dtype, hipLaunchKernelGGL(se_excite_fwd_k<T>, grid, block, 0, (hipStream_t)stream, (const T*)x, ldx,
                                          (const T*)s_, (T*)y, ldy, (int)HW, C, c_valid, g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" size_t seg_se_excite_bwd_workspace(int N, int H, int W, int C) {
    return seg_se_squeeze_workspace(N, H, W, C);
}

extern "C" int seg_se_excite_bwd(const void* x, int ldx, const void* s_, const void* dy, int lddy, void* dx, int lddx,
                                 void* ds, int N, int H, int W, int C, int c_valid, int flags, void* ws,
                                 size_t ws_bytes, int dtype, void* stream) {
    long HW;
    int st = se_status(N, H, W, C, c_valid, dtype, &HW);
    if (st != SEG_OK) return st;
    if ((st = view_status(x, (long)N * HW, ldx, C, dtype)) != SEG_OK ||
        (st = view_status(dy, (long)N * HW, lddy, C, dtype)) != SEG_OK ||
        (st = view_status(dx, (long)N * HW, lddx, C, dtype)) != SEG_OK)
        return st;
    if (!s_ || !aligned16(s_) || !ds || !aligned16(ds) || !ws || !aligned16(ws) || (flags & ~2)) return SEG_EINVAL;
    if (ws_bytes < seg_se_excite_bwd_workspace(N, H, W, C)) return SEG_EWORKSPACE;
    const Geom g = geom_of(C, epc_of(dtype));
    const int slices = se_slices(HW);
    const int per = (int)((HW + slices - 1) / slices);
    const dim3 grid(g.groups, slices, N), block(256);
    hipStream_t s = (hipStream_t)stream;
    MB_DISPATCH(dtype, hipLaunchKernelGGL((se_sum_k<T, 1>), grid, block, 0, s, (const T*)x, ldx, (const T*)s_,
                                          (const T*)dy, lddy, (T*)dx, lddx, (float*)ws, (int)HW, C, c_valid, per,
                                          (flags & 2) ? 1 : 0, g));
    SEG_CHECK_LAUNCH();
    MB_DISPATCH(dtype, hipLaunchKernelGGL(se_finish_k<T>, dim3(C / 8, N), dim3(256), 0, s,
                                          (const float*)ws, slices, C, c_valid, 1.0f, (T*)ds));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}
