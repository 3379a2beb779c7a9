// The two elementwise forms of the TransNet block
// (Network/model/FCDenseNet_TransNet.py:70-86) that are not a convolution:
//   film:  y = relu?((alpha + alpha_bias) * f + beta)    (:82-83, alpha_bias = 1)
//   axpy:  y = relu?(a + lam * b)                         (:85, lam = 0.1)
// and their gradients.  Each is one pass: HBM-bound VALU kernels on NHWC with a
// pixel stride per operand (the operands may be channel slices of a concat
// buffer), 16-byte chunks per lane, fp32 arithmetic rounded once, vector loads
// and stores only.  No reduction, so no atomics, no workspace and no LDS, and
// the results are bit-identical from run to run.
//
// Geometry (mbconv.hip's): the C / EPC chunks of a pixel are cut into `groups`
// chunk groups of LPP chunks (blockIdx.x); the 256 lanes of a workgroup are
// rows x LPP, a lane keeps its chunk and walks pixels gridDim.y * rows apart.
// The grid is capped at 2048 workgroups and strided over the rest.
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ uint4 ldc(const T* p) { return *reinterpret_cast<const uint4*>(p); }
template <typename T>
__device__ __forceinline__ void stc(T* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }

constexpr long LIMIT = 1L << 31;
constexpr int GRID_CAP = 2048;  // workgroups of a launch, at most (256 CUs x 8)

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

// y = relu?((alpha + ab) * f + beta)
template <typename T>
__global__ __launch_bounds__(256) void film_fwd_k(const T* __restrict__ alpha, int lda, const T* __restrict__ f,
                                                  int ldf, const T* __restrict__ beta, int ldb, T* __restrict__ y,
                                                  int ldy, float ab, int P, int cv, int relu, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
        float a[EPC], fv[EPC], b[EPC];
        Chunk<T>::unpack(ldc(alpha + (long)pix * lda + c0), a);
        Chunk<T>::unpack(ldc(f + (long)pix * ldf + c0), fv);
        Chunk<T>::unpack(ldc(beta + (long)pix * ldb + c0), b);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float z = __builtin_fmaf(a[e] + ab, fv[e], b[e]);
            const float o = relu ? (z > 0.f ? z : 0.f) : z;
            a[e] = c0 + e < cv ? o : 0.f;                 // padding channels: exact zeros
        }
        stc(y + (long)pix * ldy + c0, Chunk<T>::pack(a));
    }
}

// dz = dy * (y > 0) (relu) or dy; dalpha (+)= dz * f; df (+)= dz * (alpha + ab);
// dbeta (+)= dz.  A null output is skipped (and its operand not read).
template <typename T>
__global__ __launch_bounds__(256) void film_bwd_k(const T* __restrict__ dy, int lddy, const T* __restrict__ y, int ldy,
                                                  const T* __restrict__ alpha, int lda, const T* __restrict__ f,
                                                  int ldf, T* __restrict__ dalpha, int ldda, T* __restrict__ df,
                                                  int lddf, T* __restrict__ dbeta, int lddb, float ab, int P, int cv,
                                                  int flags, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    const bool relu = flags & 1, acc_a = flags & 2, acc_f = flags & 4, acc_b = flags & 8;
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
        float dz[EPC], v[EPC], o[EPC], old[EPC];
        Chunk<T>::unpack(ldc(dy + (long)pix * lddy + c0), dz);
        if (relu) {
            Chunk<T>::unpack(ldc(y + (long)pix * ldy + c0), v);
#pragma unroll
            for (int e = 0; e < EPC; ++e) dz[e] = v[e] > 0.f ? dz[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e)
            if (c0 + e >= cv) dz[e] = 0.f;
        if (dalpha) {
            Chunk<T>::unpack(ldc(f + (long)pix * ldf + c0), v);
            if (acc_a) Chunk<T>::unpack(ldc(dalpha + (long)pix * ldda + c0), old);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                o[e] = dz[e] * v[e];
                if (acc_a) o[e] += old[e];
                if (c0 + e >= cv) o[e] = 0.f;             // whatever the padding of f and dalpha holds
            }
            stc(dalpha + (long)pix * ldda + c0, Chunk<T>::pack(o));
        }
        if (df) {
            Chunk<T>::unpack(ldc(alpha + (long)pix * lda + c0), v);
            if (acc_f) Chunk<T>::unpack(ldc(df + (long)pix * lddf + c0), old);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                o[e] = dz[e] * (v[e] + ab);
                if (acc_f) o[e] += old[e];
                if (c0 + e >= cv) o[e] = 0.f;
            }
            stc(df + (long)pix * lddf + c0, Chunk<T>::pack(o));
        }
        if (dbeta) {
            if (acc_b) {
                Chunk<T>::unpack(ldc(dbeta + (long)pix * lddb + c0), old);
#pragma unroll
                for (int e = 0; e < EPC; ++e) dz[e] = c0 + e < cv ? dz[e] + old[e] : 0.f;
            }
            stc(dbeta + (long)pix * lddb + c0, Chunk<T>::pack(dz));
        }
    }
}

// y = relu?(a + lam * b)
template <typename T>
__global__ __launch_bounds__(256) void axpy_relu_fwd_k(const T* __restrict__ a, int lda, const T* __restrict__ b,
                                                       int ldb, T* __restrict__ y, int ldy, float lam, int P, int cv,
                                                       int relu, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
        float av[EPC], bv[EPC];
        Chunk<T>::unpack(ldc(a + (long)pix * lda + c0), av);
        Chunk<T>::unpack(ldc(b + (long)pix * ldb + c0), bv);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float z = __builtin_fmaf(lam, bv[e], av[e]);
            const float o = relu ? (z > 0.f ? z : 0.f) : z;
            av[e] = c0 + e < cv ? o : 0.f;
        }
        stc(y + (long)pix * ldy + c0, Chunk<T>::pack(av));
    }
}

// dz = dy * (y > 0) (relu) or dy; da (+)= dz; db (+)= lam * dz
template <typename T>
__global__ __launch_bounds__(256) void axpy_relu_bwd_k(const T* __restrict__ dy, int lddy, const T* __restrict__ y,
                                                       int ldy, T* __restrict__ da, int ldda, T* __restrict__ db,
                                                       int lddb, float lam, int P, int cv, int flags, Geom g) {
    constexpr int EPC = dt_traits<T>::EPC;
    const int cl = threadIdx.x % g.LPP, prow = threadIdx.x / g.LPP;
    const int chunk = blockIdx.x * g.LPP + cl;
    if (prow >= g.rows || chunk >= g.CK) return;
    const int c0 = chunk * EPC;
    const bool relu = flags & 1, acc_a = flags & 2, acc_b = flags & 4;
    const int step = gridDim.y * g.rows;
    for (int pix = blockIdx.y * g.rows + prow; pix < P; pix += step) {
        float dz[EPC], v[EPC], o[EPC], old[EPC];
        Chunk<T>::unpack(ldc(dy + (long)pix * lddy + c0), dz);
        if (relu) {
            Chunk<T>::unpack(ldc(y + (long)pix * ldy + c0), v);
#pragma unroll
            for (int e = 0; e < EPC; ++e) dz[e] = v[e] > 0.f ? dz[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e)
            if (c0 + e >= cv) dz[e] = 0.f;
        if (db) {
            if (acc_b) Chunk<T>::unpack(ldc(db + (long)pix * lddb + c0), old);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                o[e] = lam * dz[e];
                if (acc_b) o[e] += old[e];
                if (c0 + e >= cv) o[e] = 0.f;
            }
            stc(db + (long)pix * lddb + c0, Chunk<T>::pack(o));
        }
        if (da) {
            if (acc_a) {
                Chunk<T>::unpack(ldc(da + (long)pix * ldda + c0), old);
#pragma unroll
                for (int e = 0; e < EPC; ++e) dz[e] = c0 + e < cv ? dz[e] + old[e] : 0.f;
            }
            stc(da + (long)pix * ldda + c0, Chunk<T>::pack(dz));
        }
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

// pixel rows of the grid: one sweep covers grid.y * g.rows pixels
int walk_rows(long P, const Geom& g) {
    const long r = (P + g.rows - 1) / g.rows;
    const long cap = std::max(1, GRID_CAP / g.groups);
    return (int)(r < 1 ? 1 : r > cap ? cap : r);
}

#define TN_DISPATCH(dtype, ...)                               \
    do {                                                      \
        if ((dtype) == SEG_BF16) { using T = bf16; __VA_ARGS__; } \
        else if ((dtype) == SEG_F16) { using T = f16; __VA_ARGS__; } \
        else { using T = float; __VA_ARGS__; }               \
    } while (0)

}  // namespace

extern "C" int seg_film_fwd(const void* alpha, int lda, const void* f, int ldf, const void* beta, int ldb, void* y,
                            int ldy, float alpha_bias, long P, int C, int c_valid, int relu, int dtype,
                            void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((st = view_status(alpha, P, lda, C, dtype)) != SEG_OK || (st = view_status(f, P, ldf, C, dtype)) != SEG_OK ||
        (st = view_status(beta, P, ldb, C, dtype)) != SEG_OK || (st = view_status(y, P, ldy, C, dtype)) != SEG_OK)
        return st;
    if (relu & ~1) return SEG_EINVAL;
    const Geom g = geom_of(C, epc_of(dtype));
    const dim3 grid(g.groups, walk_rows(P, g)), block(256);
    TN_DISPATCH(dtype, hipLaunchKernelGGL(film_fwd_k<T>, grid, block, 0, (hipStream_t)stream, (const T*)alpha, lda,
                                          (const T*)f, ldf, (const T*)beta, ldb, (T*)y, ldy, alpha_bias, (int)P,
                                          c_valid, relu, g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" int seg_film_bwd(const void* dy, int lddy, const void* y, int ldy, const void* alpha, int lda,
                            const void* f, int ldf, void* dalpha, int ldda, void* df, int lddf, void* dbeta, int lddb,
                            float alpha_bias, long P, int C, int c_valid, int flags, int dtype, void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((flags & ~15) || (!dalpha && !df && !dbeta)) return SEG_EINVAL;
    if ((st = view_status(dy, P, lddy, C, dtype)) != SEG_OK) return st;
    // an operand is needed only by the output that reads it
    if ((flags & 1) && (st = view_status(y, P, ldy, C, dtype)) != SEG_OK) return st;
    if (dalpha && ((st = view_status(f, P, ldf, C, dtype)) != SEG_OK ||
                   (st = view_status(dalpha, P, ldda, C, dtype)) != SEG_OK))
        return st;
    if (df && ((st = view_status(alpha, P, lda, C, dtype)) != SEG_OK ||
               (st = view_status(df, P, lddf, C, dtype)) != SEG_OK))
        return st;
    if (dbeta && (st = view_status(dbeta, P, lddb, C, dtype)) != SEG_OK) return st;
    const Geom g = geom_of(C, epc_of(dtype));
    const dim3 grid(g.groups, walk_rows(P, g)), block(256);
    TN_DISPATCH(dtype, hipLaunchKernelGGL(film_bwd_k<T>, grid, block, 0, (hipStream_t)stream, (const T*)dy, lddy,
                                          (const T*)y, ldy, (const T*)alpha, lda, (const T*)f, ldf, (T*)dalpha, ldda,
                                          (T*)df, lddf, (T*)dbeta, lddb, alpha_bias, (int)P, c_valid, flags, g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" int seg_axpy_relu_fwd(const void* a, int lda, const void* b, int ldb, void* y, int ldy, float lam, long P,
                                 int C, int c_valid, int relu, int dtype, void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((st = view_status(a, P, lda, C, dtype)) != SEG_OK || (st = view_status(b, P, ldb, C, dtype)) != SEG_OK ||
        (st = view_status(y, P, ldy, C, dtype)) != SEG_OK)
        return st;
    if (relu & ~1) return SEG_EINVAL;
    const Geom g = geom_of(C, epc_of(dtype));
    const dim3 grid(g.groups, walk_rows(P, g)), block(256);
    TN_DISPATCH(dtype, hipLaunchKernelGGL(axpy_relu_fwd_k<T>, grid, block, 0, (hipStream_t)stream, (const T*)a, lda,
                                          (const T*)b, ldb, (T*)y, ldy, lam, (int)P, c_valid, relu, g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}

extern "C" int seg_axpy_relu_bwd(const void* dy, int lddy, const void* y, int ldy, void* da, int ldda, void* db,
                                 int lddb, float lam, long P, int C, int c_valid, int flags, int dtype,
                                 void* stream) {
    int st = chan_status(P, C, c_valid, dtype);
    if (st != SEG_OK) return st;
    if ((flags & ~7) || (!da && !db)) return SEG_EINVAL;
    if ((st = view_status(dy, P, lddy, C, dtype)) != SEG_OK) return st;
    if ((flags & 1) && (st = view_status(y, P, ldy, C, dtype)) != SEG_OK) return st;
    if (da && (st = view_status(da, P, ldda, C, dtype)) != SEG_OK) return st;
    if (db && (st = view_status(db, P, lddb, C, dtype)) != SEG_OK) return st;
    const Geom g = geom_of(C, epc_of(dtype));
    const dim3 grid(g.groups, walk_rows(P, g)), block(256);
    TN_DISPATCH(dtype, hipLaunchKernelGGL(axpy_relu_bwd_k<T>, grid, block, 0, (hipStream_t)stream, (const T*)dy, lddy,
                                          (const T*)y, ldy, (T*)da, ldda, (T*)db, lddb, lam, (int)P, c_valid, flags,
                                          g));
    SEG_CHECK_LAUNCH();
    return SEG_OK;
}
