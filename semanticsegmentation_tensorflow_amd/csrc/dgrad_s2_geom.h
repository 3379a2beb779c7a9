// Index math of dgrad_s2 (csrc/dgrad_s2.hip): the halo-tiled
// Conv2DBackpropInput of a 4x4 stride-2 Conv2D.  Plain C++ shared by the
// kernel, the host-side seg_conv2d_bwd_data_s2_ok and the stand-alone CPU
// program of tests/test_dgrad_s2_geom.py, which exhausts it.
//
// Padded coordinates: u = ih + pad_top, v = iw + pad_left.  The conv's window
// oh covers u = 2 oh + r, so an input pixel of phase (ph, pw) = (u & 1, v & 1)
// meets the taps r = ph + 2 jr, s = pw + 2 js (jr, js in {0, 1}) at
// oh = (u >> 1) - jr, ow = (v >> 1) - js.  A tile is TH x TW padded
// coordinates with an even origin, i.e. TH/2 x TW/2 pixels of each phase; its
// dy halo is rows (u0 >> 1) - 1 .. (u0 >> 1) + TH/2 - 1 and the same in v:
// (TH/2 + 1) x (TW/2 + 1) pixels.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DG2_HD __host__ __device__ inline
#else
#define DG2_HD inline
#endif

namespace dg2 {

constexpr int R = 4, S = 4, STRIDE = 2;
constexpr int TH = 8, TW = 32;                 // tile, padded coordinates
constexpr int PH = TH / 2, PW = TW / 2;        // pixels of one phase per tile: 4 rows of 16
constexpr int HH = PH + 1, HWD = PW + 1;       // dy halo: 5 x 17 pixels
constexpr int HPIX = HH * HWD;
constexpr int CB = 32;                         // dx channels per block
constexpr int KMAX = 256;                      // dy channels staged per halo pixel
constexpr unsigned OOB = 0x80000000u;          // buffer offset that reads as zero

static_assert(PW == 16, "one MFMA fragment = the 16 pixels of one phase row");
static_assert(TH % 2 == 0 && TW % 2 == 0, "tile origin keeps the stride phase");

// LDS row of one halo pixel: K/8 16-byte chunks + one pad chunk (the fragment
// read of 16 consecutive pixels then strides 2K + 16 bytes, not a multiple of
// the 256-byte bank period)
DG2_HD int row_chunks(int K) { return K / 8 + 1; }
DG2_HD int halo_chunks(int K) { return HPIX * row_chunks(K); }
// LDS bytes, whole 1 KiB DMA pieces
DG2_HD int lds_bytes(int K) { return (halo_chunks(K) + 63) / 64 * 1024; }

DG2_HD int tiles_y(int H, int pad_top) { return (H + pad_top + TH - 1) / TH; }
DG2_HD int tiles_x(int W, int pad_left) { return (W + pad_left + TW - 1) / TW; }

// Source of LDS chunk q of the tile at padded origin (u0, v0): the byte
// offset inside one image of dy ([OH][OW][ldy] 16-bit elements), or OOB for
// the pad chunk, chunks past the halo and pixels outside the map.
DG2_HD unsigned halo_src(int q, int u0, int v0, int OH, int OW, int ldy, int K) {
    const int rc = row_chunks(K);
    const int hp = q / rc, kc = q - hp * rc;
    if (hp >= HPIX || kc >= K / 8) return OOB;
    const int hr = hp / HWD, hc = hp - hr * HWD;
    const int oh = (u0 >> 1) - 1 + hr, ow = (v0 >> 1) - 1 + hc;
    if (oh < 0 || oh >= OH || ow < 0 || ow >= OW) return OOB;
    return (unsigned)(((oh * OW + ow) * ldy + kc * 8) * 2);
}

// Halo pixel (row-major index into the 5 x 17 halo) that phase-row i, phase
// column j reads for tap (jr, js)
DG2_HD int halo_pix(int i, int j, int jr, int js) { return (i + 1 - jr) * HWD + (j + 1 - js); }

// Input pixel of slot (phase ph/pw, phase-row i, phase column j) of the tile at
// (u0, v0); the slot stores only when 0 <= ih < H and 0 <= iw < W
DG2_HD int slot_ih(int u0, int ph, int i, int pad_top) { return u0 + 2 * i + ph - pad_top; }
DG2_HD int slot_iw(int v0, int pw, int j, int pad_left) { return v0 + 2 * j + pw - pad_left; }

// Shape part of seg_conv2d_bwd_data_s2_ok (dtype checked by the caller):
// 4x4 / 2, no dilation, padded channel counts that tile the MFMA fragments,
// offsets that fit the 31-bit buffer offset.
DG2_HD bool shape_ok(int N, int H, int W, int C, int OH, int OW, int K, int Rr, int Ss, int sh, int sw, int dh, int dw,
                     int pad_top, int pad_left, int ldx, int ldy) {
    if (Rr != R || Ss != S || sh != STRIDE || sw != STRIDE || dh != 1 || dw != 1) return false;
    if (K % 32 || K > KMAX || K <= 0) return false;
    if (!(C == 16 || (C > 0 && C % CB == 0))) return false;
    if (pad_top < 0 || pad_top > 1 || pad_left < 0 || pad_left > 1) return false;
    if (ldy < K || ldx < C || (ldy & 7) || (ldx & 7)) return false;
    if ((long)OH * OW * ldy * 2 >= (1L << 31)) return false;
    if ((long)N * tiles_y(H, pad_top) * tiles_x(W, pad_left) >= (1L << 31)) return false;
    return true;
}

}  // namespace dg2
