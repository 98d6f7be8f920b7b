// Windowed multi-head self-attention (ViTDet, Li et al. 2022) for the ViT streams. gfx950 only.
//
// Token 0 is CLS, patch token 1 + r*gw + c sits at (r, c) of the gh x gw grid, and a window size
// (wh, ww) tiles the grid from the top-left corner: patch (r, c) belongs to window (r / wh, c / ww),
// the last row / column of windows is smaller when wh / ww do not divide the grid (nothing is padded,
// nothing wraps). A patch query attends to the patch keys of its own window only; CLS is a window of
// its own (o_cls = v_cls, its lse is its single score, dq_cls = dk_cls = 0, dv_cls = do_cls).
//
// One workgroup (4 waves) per (window, sample, head); a flat grid of (windows + 1) * B * H workgroups,
// the window index fastest; the extra block of each (sample, head) copies the CLS row. A window has at most 256 tokens, so its whole key set is resident:
//   * Q (backward only; the forward reads its Q fragments straight from memory), K, V and dO of the
//     window are loaded ONCE into LDS as [token][64] bf16 rows of 144 B (16-B aligned chunks, the 16
//     extra bytes spread the rows over the banks), rows from the window's token count up to the next
//     multiple of 32 zero-filled. A token outside the window is never read.
//   * scores stay in registers: S^T = K Q^T on the 16x16x32 bf16 MFMA leaves a query's row in the four
//     lanes of its column, so the softmax is a plain row softmax (one max, one sum, no rescale), masked
//     by SELECTION (key >= window size -> -big / 0), and the accumulator tile is the next product's
//     operand as it stands (its k order is the permuted one of the C layout; the other operand is
//     read from LDS in the same order with the transposing read, ds_read_b64_tr_b16).
//   * forward: O^T = V^T P^T, divided by the row sum, 8-B stores. lse = max + log2(sum) in the
//     units of the global entry of the same name (natural log for ivit_attn_win_fwd, log2 for _q2).
//   * backward, phase A (a wave owns 16 queries): S^T and dP^T = V dO^T, P normalised by the row's own
//     sum, delta = sum_k P dP, dS = P (dP - delta), dQ^T = K^T dS^T; the row constants (max + log2 sum,
//     delta) go to LDS. Phase B (a wave owns 16 keys): S = Q K^T and dP = dO V^T again for every query
//     of the window, P = exp2(S - row constant), dV^T = dO^T P, dK^T = Q^T dS. dQ, dK and dV of a window
//     come from the same workgroup: no atomics, no second kernel, no workspace, bitwise repeatable.
//     The backward reads NEITHER lse NOR out: it renormalises by the row's own sum, as the f32 global
//     backward does (both arguments are accepted for a contract that mirrors ivit_attn_bwd).
// LDS: forward 2 panels, backward 4 panels of kp x 144 B (kp = window tokens rounded up to 32) plus
// 2 x kp floats: 10x10 windows 36 / 74 KB (4 / 2 workgroups per CU), the 256-token limit 72 / 146 KB.
// VGPRs: the backward's phase A holds S^T and dP^T of 16 queries x kp keys, 2 x kp / 4 accumulators per
// lane (128 at the limit); the kernels are instantiated for kp <= 32, 64, 128, 256 and, up to kp = 128,
// bounded to 256 registers so that two workgroups share a CU (123 used at kp = 128; built with
// -fno-slp-vectorize, without which the same instantiation took 362).
// Byte floor per call: forward reads qkv and writes o (4 x B N D elements), backward reads qkv and dout
// and writes dqkv (7 x B N D elements).
//
// The f32 entries are the parity path: one thread per query (phase A) / per key (phase B), K and V (then
// Q and dO) of the window in LDS as f32, every sum in f32 FMAs in a fixed order.
#include <mutex>

#include "ivit_common.h"

namespace {

constexpr float W_LOG2E = 1.4426950408889634f;
constexpr float W_LN2 = 0.69314718055994531f;
constexpr float W_NEG_BIG = -1.0e30f;
constexpr int WROWB = 144;  // bytes per LDS row of 64 bf16

struct WinGeom {
  int gh, gw, wh, ww, nwc, nwin;
};

struct WinBox {
  int r0, c0, cols, nw;
};

IVIT_DEV WinBox win_box(const WinGeom& G, int w) {
  const int wr = w / G.nwc, wc = w - wr * G.nwc;
  WinBox x;
  x.r0 = wr * G.wh;
  x.c0 = wc * G.ww;
  x.cols = min(G.ww, G.gw - x.c0);
  x.nw = min(G.wh, G.gh - x.r0) * x.cols;
  return x;
}

// token index of element e (< nw) of the window
IVIT_DEV int win_token(const WinGeom& G, const WinBox& x, int e) {
  const int r = e / x.cols;
  return 1 + (x.r0 + r) * G.gw + x.c0 + (e - r * x.cols);
}

// [kp][64] bf16 panel of the window into LDS: rows e < nw from src + token(e) * ld, the rest zeros.
// kp is a multiple of 32, so every thread of the 256 makes the same number of trips.
IVIT_DEV void win_load(char* lds, const bf16* src, long ld, const WinGeom& G, const WinBox& x, int kp, int tid) {
  for (int i = tid; i < kp * 8; i += 256) {
    const int e = i >> 3, ch = i & 7;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (e < x.nw) v = *(const uint4*)(src + (long)win_token(G, x, e) * ld + ch * 8);
    *(uint4*)(lds + e * WROWB + ch * 16) = v;
  }
}

// 16x16x32 operand read along a row: lane (g, m) holds row[row0 + m][32 s + 8 g .. + 7]
IVIT_DEV bf16x8 win_row(const char* img, int row0, int s, int lane) {
  return *(const bf16x8*)(img + (row0 + (lane & 15)) * WROWB + 64 * s + 16 * (lane >> 4));
}

IVIT_DEV s16x4 win_ds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// 16x16x32 operand read across rows, in the k order of an accumulator tile pair: lane (g, m) holds
// img[row0 + 16 (j >> 2) + 4 g + (j & 3)][col0 + m], j = 0..7. Every lane of the wave must be active.
IVIT_DEV bf16x8 win_tr(const char* img, int row0, int col0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const char* a = img + (row0 + 4 * g + q) * WROWB + (col0 + 4 * p) * 2;
  union {
    s16x4 s[2];
    bf16x8 v;
  } u;
  u.s[0] = win_ds_tr(a);
  u.s[1] = win_ds_tr(a + 16 * WROWB);
  return u.v;
}

IVIT_DEV f32x4 win_mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

IVIT_DEV f32x4 win_zero4() {
  f32x4 a;
  a[0] = a[1] = a[2] = a[3] = 0.f;
  return a;
}

// two accumulator tiles (rows 4 g + i of tiles lo and hi) as one operand fragment
IVIT_DEV bf16x8 win_pack(const f32x4& lo, const f32x4& hi) {
  Pack8 p;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p.h[i] = (bf16)lo[i];
    p.h[4 + i] = (bf16)hi[i];
  }
  return p.v;
}

IVIT_DEV float quad_max(float v) {  // over the four lanes n, n + 16, n + 32, n + 48
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
IVIT_DEV float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// 4 accumulator values (rows d0 .. d0 + 3 of a transposed tile) -> 4 consecutive elements
IVIT_DEV void win_store4(bf16* p, const f32x4& v, float s) {
  Pack4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o.h[i] = (bf16)(v[i] * s);
  *(uint2*)p = o.u;
}

// ------------------------------------------------------------------------------- bf16 forward
template <int KT>
__global__ __launch_bounds__(256) void attn_win_fwd_bf16_kernel(const bf16* __restrict__ qkv, WinGeom G, int N, int H,
                                                                bf16* __restrict__ out, float* __restrict__ lse,
                                                                float c2, float lse_mul,
                                                                const float* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, n = lane & 15;
  const int z = blockIdx.x / (G.nwin + 1), w = blockIdx.x - z * (G.nwin + 1), b = z / H, h = z - b * H;
  const long D = (long)H * 64, ld = 3 * D;
  const bf16* base = qkv + (long)b * N * ld + h * 64;
  bf16* ob = out + (long)b * N * D + h * 64;
  float* lb = lse + (long)z * N;
  const bool drop = skip != nullptr && skip[b] == 0.0f;
  if (w == G.nwin) {  // CLS: o = v, lse = its one score
    if (wv != 0) return;
    if (drop) {
      if (lane < 8) *(uint4*)(ob + lane * 8) = make_uint4(0u, 0u, 0u, 0u);
      return;
    }
    if (lane < 8) *(uint4*)(ob + lane * 8) = *(const uint4*)(base + 2 * D + lane * 8);
    const float s = wave_sum((float)base[lane] * (float)base[D + lane]);
    if (lane == 0) lb[0] = s * c2 * lse_mul;
    return;
  }
  const WinBox x = win_box(G, w);
  if (drop) {
    for (int i = tid; i < x.nw * 8; i += 256)
      *(uint4*)(ob + (long)win_token(G, x, i >> 3) * D + (i & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const int kp = (x.nw + 31) & ~31;
  char* Ks = smem;
  char* Vs = smem + kp * WROWB;
  win_load(Ks, base + D, ld, G, x, kp, tid);
  win_load(Vs, base + 2 * D, ld, G, x, kp, tid);
  __syncthreads();
  const int nt = (x.nw + 15) >> 4;
  for (int qt = wv; qt < nt; qt += 4) {
    const int q0 = 16 * qt;
    const bool qv = q0 + n < x.nw;
    const int tok = win_token(G, x, qv ? q0 + n : 0);
    bf16x8 qf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Pack8 p;
      p.u = qv ? *(const uint4*)(base + (long)tok * ld + 32 * s + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
      qf[s] = p.v;
    }
    // S^T[key][query]: st[t][i] = key 16 t + 4 g + i, query q0 + n
    f32x4 st[2 * KT];
    float mx = W_NEG_BIG;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t) {
      st[t] = win_zero4();
      if (16 * t < kp) {
#pragma unroll
        for (int s = 0; s < 2; ++s) st[t] = win_mfma(win_row(Ks, 16 * t, s, lane), qf[s], st[t]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = 16 * t + 4 * g + i < x.nw ? st[t][i] * c2 : W_NEG_BIG;
          st[t][i] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = quad_max(mx);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (16 * t < kp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = 16 * t + 4 * g + i < x.nw ? fast_exp2(st[t][i] - mx) : 0.f;
          st[t][i] = p;
          l += p;
        }
      }
    l = quad_sum(l);
    // O^T[d][query] = sum_key V[key][d] P^T[key][query]
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = win_zero4();
#pragma unroll
    for (int jj = 0; jj < KT; ++jj)
      if (32 * jj < kp) {
        const bf16x8 pf = win_pack(st[2 * jj], st[2 * jj + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = win_mfma(win_tr(Vs, 32 * jj, 16 * dt, lane), pf, o[dt]);
      }
    if (qv) {
      const float inv = 1.0f / l;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) win_store4(ob + (long)tok * D + 16 * dt + 4 * g, o[dt], inv);
      if (g == 0) lb[tok] = (mx + log2f(l)) * lse_mul;
    }
  }
}

// ------------------------------------------------------------------------------- bf16 backward
// c2: what turns the raw q.k of the Q in memory into log2 units (1 for the prescaled Q);
// qs: dQ = qs dS K (1/8); ks: dK = ks dS^T Q (1/8 for the plain Q, ln 2 for the prescaled one).
template <int KT>
__global__ __launch_bounds__(256, KT <= 4 ? 2 : 1) void attn_win_bwd_bf16_kernel(const bf16* __restrict__ qkv,
                                                                const bf16* __restrict__ dout, WinGeom G, int N,
                                                                int H, bf16* __restrict__ dqkv, float c2, float qs,
                                                                float ks, const float* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, n = lane & 15;
  const int z = blockIdx.x / (G.nwin + 1), w = blockIdx.x - z * (G.nwin + 1), b = z / H, h = z - b * H;
  const long D = (long)H * 64, ld = 3 * D;
  const bf16* base = qkv + (long)b * N * ld + h * 64;
  const bf16* dob = dout + (long)b * N * D + h * 64;
  bf16* gb = dqkv + (long)b * N * ld + h * 64;
  const bool drop = skip != nullptr && skip[b] == 0.0f;
  if (w == G.nwin) {  // CLS: dq = dk = 0, dv = do
    if (wv != 0) return;
    if (lane < 24) {
      const int part = lane >> 3, ch = lane & 7;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (part == 2 && !drop) v = *(const uint4*)(dob + ch * 8);
      *(uint4*)(gb + part * D + ch * 8) = v;
    }
    return;
  }
  const WinBox x = win_box(G, w);
  if (drop) {
    for (int i = tid; i < x.nw * 24; i += 256) {
      const int e = i / 24, r = i - 24 * e;
      *(uint4*)(gb + (long)win_token(G, x, e) * ld + (r >> 3) * D + (r & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const int kp = (x.nw + 31) & ~31;
  char* Qs = smem;
  char* Ks = Qs + kp * WROWB;
  char* Vs = Ks + kp * WROWB;
  char* Os = Vs + kp * WROWB;
  float* rlse = (float*)(Os + kp * WROWB);  // [kp] max + log2(sum) of a query's row
  float* rdel = rlse + kp;                  // [kp] delta
  win_load(Qs, base, ld, G, x, kp, tid);
  win_load(Ks, base + D, ld, G, x, kp, tid);
  win_load(Vs, base + 2 * D, ld, G, x, kp, tid);
  win_load(Os, dob, D, G, x, kp, tid);
  for (int i = tid; i < 2 * kp; i += 256) rlse[i] = 0.f;
  __syncthreads();
  const int nt = (x.nw + 15) >> 4;
  // ---- phase A: dQ of 16 queries per wave trip
  for (int qt = wv; qt < nt; qt += 4) {
    const int q0 = 16 * qt;
    const bool qv = q0 + n < x.nw;
    bf16x8 qf[2], of[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[s] = win_row(Qs, q0, s, lane);
      of[s] = win_row(Os, q0, s, lane);
    }
    f32x4 st[2 * KT], dp[2 * KT];
    float mx = W_NEG_BIG;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t) {
      st[t] = win_zero4();
      dp[t] = win_zero4();
      if (16 * t < kp) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          st[t] = win_mfma(win_row(Ks, 16 * t, s, lane), qf[s], st[t]);
          dp[t] = win_mfma(win_row(Vs, 16 * t, s, lane), of[s], dp[t]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = 16 * t + 4 * g + i < x.nw ? st[t][i] * c2 : W_NEG_BIG;
          st[t][i] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = quad_max(mx);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (16 * t < kp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = 16 * t + 4 * g + i < x.nw ? fast_exp2(st[t][i] - mx) : 0.f;
          st[t][i] = p;
          l += p;
        }
      }
    l = quad_sum(l);
    const float inv = 1.0f / l;
    float del = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (16 * t < kp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool kv = 16 * t + 4 * g + i < x.nw;
          const float p = st[t][i] * inv;
          st[t][i] = p;
          del += kv ? p * dp[t][i] : 0.f;
        }
      }
    del = quad_sum(del);
    if (qv && g == 0) {
      rlse[q0 + n] = mx + log2f(l);
      rdel[q0 + n] = del;
    }
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (16 * t < kp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool kv = 16 * t + 4 * g + i < x.nw;
          st[t][i] = kv ? st[t][i] * (dp[t][i] - del) : 0.f;
        }
      }
    // dQ^T[d][query] = sum_key K[key][d] dS^T[key][query]
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = win_zero4();
#pragma unroll
    for (int jj = 0; jj < KT; ++jj)
      if (32 * jj < kp) {
        const bf16x8 sf = win_pack(st[2 * jj], st[2 * jj + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = win_mfma(win_tr(Ks, 32 * jj, 16 * dt, lane), sf, dq[dt]);
      }
    if (qv) {
      const int tok = win_token(G, x, q0 + n);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) win_store4(gb + (long)tok * ld + 16 * dt + 4 * g, dq[dt], qs);
    }
  }
  __syncthreads();
  // ---- phase B: dK and dV of 16 keys per wave trip
  for (int kt = wv; kt < nt; kt += 4) {
    const int k0 = 16 * kt;
    const bool kv = k0 + n < x.nw;
    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[s] = win_row(Ks, k0, s, lane);
      vf[s] = win_row(Vs, k0, s, lane);
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dk[dt] = win_zero4();
      dv[dt] = win_zero4();
    }
    for (int jj = 0; 32 * jj < kp; ++jj) {
      // S[query][key]: row 32 jj + 16 u + 4 g + i, column k0 + n
      f32x4 pp[2], ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r0 = 32 * jj + 16 * u;
        f32x4 s4 = win_zero4(), d4 = win_zero4();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          s4 = win_mfma(win_row(Qs, r0, s, lane), kf[s], s4);
          d4 = win_mfma(win_row(Os, r0, s, lane), vf[s], d4);
        }
        const float4 rl = *(const float4*)(rlse + r0 + 4 * g);
        const float4 rd = *(const float4*)(rdel + r0 + 4 * g);
        const float rls[4] = {rl.x, rl.y, rl.z, rl.w}, rds[4] = {rd.x, rd.y, rd.z, rd.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = kv && r0 + 4 * g + i < x.nw;
          const float p = ok ? fast_exp2(s4[i] * c2 - rls[i]) : 0.f;
          pp[u][i] = p;
          ds[u][i] = ok ? p * (d4[i] - rds[i]) : 0.f;
        }
      }
      const bf16x8 pf = win_pack(pp[0], pp[1]), sf = win_pack(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dv[dt] = win_mfma(win_tr(Os, 32 * jj, 16 * dt, lane), pf, dv[dt]);
        dk[dt] = win_mfma(win_tr(Qs, 32 * jj, 16 * dt, lane), sf, dk[dt]);
      }
    }
    if (kv) {
      const int tok = win_token(G, x, k0 + n);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        win_store4(gb + (long)tok * ld + D + 16 * dt + 4 * g, dk[dt], ks);
        win_store4(gb + (long)tok * ld + 2 * D + 16 * dt + 4 * g, dv[dt], 1.0f);
      }
    }
  }
}

// ------------------------------------------------------------------------------- f32 parity path
IVIT_DEV void win_load_f32(float* lds, const float* src, long ld, const WinGeom& G, const WinBox& x, int tid) {
  for (int i = tid; i < x.nw * 16; i += 256) {
    const int e = i >> 4, ch = i & 15;
    *(float4*)(lds + e * 64 + ch * 4) = *(const float4*)(src + (long)win_token(G, x, e) * ld + ch * 4);
  }
}

IVIT_DEV float win_dot64(const float (&a)[64], const float* __restrict__ r) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 64; ++d) s = fmaf(a[d], r[d], s);
  return s;
}

IVIT_DEV void win_ld64(float (&a)[64], const float* p) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const float4 v = *(const float4*)(p + 4 * c);
    a[4 * c] = v.x;
    a[4 * c + 1] = v.y;
    a[4 * c + 2] = v.z;
    a[4 * c + 3] = v.w;
  }
}

IVIT_DEV void win_st64(float* p, const float (&a)[64], float s) {
#pragma unroll
  for (int c = 0; c < 16; ++c)
    *(float4*)(p + 4 * c) = make_float4(a[4 * c] * s, a[4 * c + 1] * s, a[4 * c + 2] * s, a[4 * c + 3] * s);
}

__global__ __launch_bounds__(256) void attn_win_fwd_f32_kernel(const float* __restrict__ qkv, WinGeom G, int N, int H,
                                                               float* __restrict__ out, float* __restrict__ lse,
                                                               float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int z = blockIdx.x / (G.nwin + 1), w = blockIdx.x - z * (G.nwin + 1), b = z / H, h = z - b * H;
  const long D = (long)H * 64, ld = 3 * D;
  const float* base = qkv + (long)b * N * ld + h * 64;
  float* ob = out + (long)b * N * D + h * 64;
  float* lb = lse + (long)z * N;
  if (w == G.nwin) {
    if (tid >= 64) return;
    ob[tid] = base[2 * D + tid];
    const float s = wave_sum(base[tid] * base[D + tid]);
    if (tid == 0) lb[0] = s * scale;
    return;
  }
  const WinBox x = win_box(G, w);
  float* Ks = (float*)smem;
  float* Vs = Ks + x.nw * 64;
  win_load_f32(Ks, base + D, ld, G, x, tid);
  win_load_f32(Vs, base + 2 * D, ld, G, x, tid);
  __syncthreads();
  if (tid >= x.nw) return;
  const int tok = win_token(G, x, tid);
  float q[64], o[64];
  win_ld64(q, base + (long)tok * ld);
  float mx = W_NEG_BIG;
  for (int k = 0; k < x.nw; ++k) mx = fmaxf(mx, win_dot64(q, Ks + k * 64) * scale);
#pragma unroll
  for (int d = 0; d < 64; ++d) o[d] = 0.f;
  float l = 0.f;
  for (int k = 0; k < x.nw; ++k) {
    const float p = expf(win_dot64(q, Ks + k * 64) * scale - mx);
    l += p;
#pragma unroll
    for (int d = 0; d < 64; ++d) o[d] = fmaf(p, Vs[k * 64 + d], o[d]);
  }
  win_st64(ob + (long)tok * D, o, 1.0f / l);
  lb[tok] = mx + logf(l);
}

__global__ __launch_bounds__(256) void attn_win_bwd_f32_kernel(const float* __restrict__ qkv,
                                                               const float* __restrict__ dout, WinGeom G, int N,
                                                               int H, float* __restrict__ dqkv, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int z = blockIdx.x / (G.nwin + 1), w = blockIdx.x - z * (G.nwin + 1), b = z / H, h = z - b * H;
  const long D = (long)H * 64, ld = 3 * D;
  const float* base = qkv + (long)b * N * ld + h * 64;
  const float* dob = dout + (long)b * N * D + h * 64;
  float* gb = dqkv + (long)b * N * ld + h * 64;
  if (w == G.nwin) {
    if (tid >= 64) return;
    gb[tid] = 0.f;
    gb[D + tid] = 0.f;
    gb[2 * D + tid] = dob[tid];
    return;
  }
  const WinBox x = win_box(G, w);
  float* A0 = (float*)smem;        // K, then Q
  float* A1 = A0 + x.nw * 64;      // V, then dO
  float* rmx = A1 + x.nw * 64;     // [nw] row max
  float* rinv = rmx + x.nw;        // [nw] 1 / row sum
  float* rdel = rinv + x.nw;       // [nw] delta
  win_load_f32(A0, base + D, ld, G, x, tid);
  win_load_f32(A1, base + 2 * D, ld, G, x, tid);
  __syncthreads();
  const bool mine = tid < x.nw;
  const int tok = win_token(G, x, mine ? tid : 0);
  {  // phase A: this thread's query
    float q[64], go[64], dq[64];
    if (mine) {
      win_ld64(q, base + (long)tok * ld);
      win_ld64(go, dob + (long)tok * D);
      float mx = W_NEG_BIG;
      for (int k = 0; k < x.nw; ++k) mx = fmaxf(mx, win_dot64(q, A0 + k * 64) * scale);
      float l = 0.f, dn = 0.f;
      for (int k = 0; k < x.nw; ++k) {
        const float e = expf(win_dot64(q, A0 + k * 64) * scale - mx);
        l += e;
        dn = fmaf(e, win_dot64(go, A1 + k * 64), dn);
      }
      const float inv = 1.0f / l, del = dn * inv;
#pragma unroll
      for (int d = 0; d < 64; ++d) dq[d] = 0.f;
      for (int k = 0; k < x.nw; ++k) {
        const float p = expf(win_dot64(q, A0 + k * 64) * scale - mx) * inv;
        const float ds = p * (win_dot64(go, A1 + k * 64) - del);
#pragma unroll
        for (int d = 0; d < 64; ++d) dq[d] = fmaf(ds, A0[k * 64 + d], dq[d]);
      }
      win_st64(gb + (long)tok * ld, dq, scale);
      rmx[tid] = mx;
      rinv[tid] = inv;
      rdel[tid] = del;
    }
  }
  __syncthreads();
  // phase B: this thread's key; Q and dO replace K and V in LDS
  float kr[64], vr[64];
  if (mine) {
    win_ld64(kr, A0 + tid * 64);
    win_ld64(vr, A1 + tid * 64);
  }
  __syncthreads();
  win_load_f32(A0, base, ld, G, x, tid);
  win_load_f32(A1, dob, D, G, x, tid);
  __syncthreads();
  if (!mine) return;
  float dk[64], dv[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) dk[d] = dv[d] = 0.f;
  for (int qi = 0; qi < x.nw; ++qi) {
    // the same products in the same order as phase A: q.k and do.v
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < 64; ++d) s = fmaf(A0[qi * 64 + d], kr[d], s);
#pragma unroll
    for (int d = 0; d < 64; ++d) dp = fmaf(A1[qi * 64 + d], vr[d], dp);
    const float p = expf(s * scale - rmx[qi]) * rinv[qi];
    const float ds = p * (dp - rdel[qi]);
#pragma unroll
    for (int d = 0; d < 64; ++d) {
      dv[d] = fmaf(p, A1[qi * 64 + d], dv[d]);
      dk[d] = fmaf(ds, A0[qi * 64 + d], dk[d]);
    }
  }
  win_st64(gb + (long)tok * ld + D, dk, scale);
  win_st64(gb + (long)tok * ld + 2 * D, dv, 1.0f);
}

// ------------------------------------------------------------------------------- launchers
struct WinLaunch {
  WinGeom G;
  int kt;        // 32-key groups the bf16 kernels are instantiated for: 1, 2, 4, 8
  int nwmax;     // tokens of the largest window
};

int win_check(const char* who, long B, long N, long gh, long gw, long wh, long ww, long H, long Dh, WinLaunch& L) {
  IVIT_CHECK_ARG(Dh == 64, "%s: head dim must be 64 (got %ld)", who, Dh);
  IVIT_CHECK_ARG(B >= 0 && H >= 1 && gh >= 1 && gw >= 1, "%s: bad sizes B %ld H %ld grid %ld x %ld", who, B, H, gh, gw);
  IVIT_CHECK_ARG(wh >= 1 && ww >= 1, "%s: window %ld x %ld must be at least 1 x 1", who, wh, ww);
  IVIT_CHECK_ARG(wh * ww <= 256, "%s: window %ld x %ld holds more than 256 tokens", who, wh, ww);
  IVIT_CHECK_ARG(N == 1 + gh * gw, "%s: N = %ld is not 1 + %ld x %ld", who, N, gh, gw);
  IVIT_CHECK_ARG((gh * gw + 1) * B * H <= 0x7fffffffL, "%s: more than 2^31 - 1 workgroups", who);
  const long nwr = (gh + wh - 1) / wh, nwc = (gw + ww - 1) / ww;
  L.G = WinGeom{(int)gh, (int)gw, (int)wh, (int)ww, (int)nwc, (int)(nwr * nwc)};
  L.nwmax = (int)((wh < gh ? wh : gh) * (ww < gw ? ww : gw));
  L.kt = L.nwmax <= 32 ? 1 : L.nwmax <= 64 ? 2 : L.nwmax <= 128 ? 4 : 8;
  return 0;
}

// Dynamic LDS above the 64-KB default needs the attribute raised, per device: once per kernel
// instantiation and device (function-local statics, so not on the per-launch path), to the most that
// instantiation can ask for.
constexpr int WIN_MAX_DEVICES = 64;
template <auto Kernel>
hipError_t win_lds_attr(size_t max_bytes) {
  static std::mutex mu;
  static bool raised[WIN_MAX_DEVICES] = {};
  if (max_bytes <= 65536) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  const bool known = dev >= 0 && dev < WIN_MAX_DEVICES;
  if (known && raised[dev]) return hipSuccess;
  e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes);
  if (e == hipSuccess && known) raised[dev] = true;
  return e;
}

#define WIN_ATTR(kernel, max_bytes)                                               \
  do {                                                                            \
    hipError_t e_ = win_lds_attr<kernel>(max_bytes);                              \
    if (e_ != hipSuccess) {                                                       \
      ivit_set_error("%s: LDS attribute: %s", __func__, hipGetErrorString(e_));   \
      return (int)e_;                                                             \
    }                                                                             \
  } while (0)

constexpr size_t win_fwd_lds(int kp) { return (size_t)2 * kp * WROWB; }
constexpr size_t win_bwd_lds(int kp) { return (size_t)4 * kp * WROWB + (size_t)2 * kp * 4; }
constexpr size_t WIN_F32_FWD_LDS = (size_t)2 * 256 * 64 * 4;
constexpr size_t WIN_F32_BWD_LDS = (size_t)(2 * 256 * 64 + 3 * 256) * 4;

const float* win_drop_skip(const float* skip) { return ivit_knob(IVIT_KNOB_DROP_SKIP) != 0 ? skip : nullptr; }

template <int KT>
int win_fwd_bf16(const WinLaunch& L, const void* qkv, long B, long N, long H, void* out, float* lse, float c2,
                 float lse_mul, const float* skip, hipStream_t st) {
  const int kp = (L.nwmax + 31) & ~31;
  const size_t bytes = win_fwd_lds(kp);
  WIN_ATTR(attn_win_fwd_bf16_kernel<KT>, win_fwd_lds(32 * KT));
  hipLaunchKernelGGL(attn_win_fwd_bf16_kernel<KT>, dim3((unsigned)((L.G.nwin + 1) * B * H)), dim3(256), bytes, st,
                     (const bf16*)qkv, L.G, (int)N, (int)H, (bf16*)out, lse, c2, lse_mul, skip);
  IVIT_LAUNCH_CHECK();
  return 0;
}

template <int KT>
int win_bwd_bf16(const WinLaunch& L, const void* qkv, const void* dout, long B, long N, long H, void* dqkv, float c2,
                 float ks, const float* skip, hipStream_t st) {
  const int kp = (L.nwmax + 31) & ~31;
  const size_t bytes = win_bwd_lds(kp);
  WIN_ATTR(attn_win_bwd_bf16_kernel<KT>, win_bwd_lds(32 * KT));
  hipLaunchKernelGGL(attn_win_bwd_bf16_kernel<KT>, dim3((unsigned)((L.G.nwin + 1) * B * H)), dim3(256), bytes, st,
                     (const bf16*)qkv, (const bf16*)dout, L.G, (int)N, (int)H, (bf16*)dqkv, c2, 0.125f, ks, skip);
  IVIT_LAUNCH_CHECK();
  return 0;
}

int win_fwd_bf16_any(const WinLaunch& L, const void* qkv, long B, long N, long H, void* out, float* lse, float c2,
                     float lse_mul, const float* skip, hipStream_t st) {
  switch (L.kt) {
    case 1: return win_fwd_bf16<1>(L, qkv, B, N, H, out, lse, c2, lse_mul, skip, st);
    case 2: return win_fwd_bf16<2>(L, qkv, B, N, H, out, lse, c2, lse_mul, skip, st);
    case 4: return win_fwd_bf16<4>(L, qkv, B, N, H, out, lse, c2, lse_mul, skip, st);
    default: return win_fwd_bf16<8>(L, qkv, B, N, H, out, lse, c2, lse_mul, skip, st);
  }
}

int win_bwd_bf16_any(const WinLaunch& L, const void* qkv, const void* dout, long B, long N, long H, void* dqkv,
                     float c2, float ks, const float* skip, hipStream_t st) {
  switch (L.kt) {
    case 1: return win_bwd_bf16<1>(L, qkv, dout, B, N, H, dqkv, c2, ks, skip, st);
    case 2: return win_bwd_bf16<2>(L, qkv, dout, B, N, H, dqkv, c2, ks, skip, st);
    case 4: return win_bwd_bf16<4>(L, qkv, dout, B, N, H, dqkv, c2, ks, skip, st);
    default: return win_bwd_bf16<8>(L, qkv, dout, B, N, H, dqkv, c2, ks, skip, st);
  }
}

}  // namespace

extern "C" int ivit_attn_win_fwd(int dtype, const void* qkv, long B, long N, long gh, long gw, long wh, long ww, long H,
                                 long Dh, void* out, float* lse, void* stream) {
  WinLaunch L;
  if (int rc = win_check("ivit_attn_win_fwd", B, N, gh, gw, wh, ww, H, Dh, L)) return rc;
  IVIT_CHECK_ARG(dtype == IVIT_F32 || dtype == IVIT_BF16, "ivit_attn_win_fwd: unknown dtype %d", dtype);
  if (B == 0) return 0;
  hipStream_t st = ivit_stream(stream);
  if (dtype == IVIT_BF16)
    return win_fwd_bf16_any(L, qkv, B, N, H, out, lse, 0.125f * W_LOG2E, W_LN2, nullptr, st);
  const size_t bytes = (size_t)2 * L.nwmax * 64 * 4;
  WIN_ATTR(attn_win_fwd_f32_kernel, WIN_F32_FWD_LDS);
  hipLaunchKernelGGL(attn_win_fwd_f32_kernel, dim3((unsigned)((L.G.nwin + 1) * B * H)), dim3(256), bytes, st,
                     (const float*)qkv, L.G, (int)N, (int)H, (float*)out, lse, 0.125f);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_attn_win_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, long B,
                                 long N, long gh, long gw, long wh, long ww, long H, long Dh, void* dqkv,
                                 void* stream) {
  (void)out;
  (void)lse;
  WinLaunch L;
  if (int rc = win_check("ivit_attn_win_bwd", B, N, gh, gw, wh, ww, H, Dh, L)) return rc;
  IVIT_CHECK_ARG(dtype == IVIT_F32 || dtype == IVIT_BF16, "ivit_attn_win_bwd: unknown dtype %d", dtype);
  if (B == 0) return 0;
  hipStream_t st = ivit_stream(stream);
  if (dtype == IVIT_BF16) return win_bwd_bf16_any(L, qkv, dout, B, N, H, dqkv, 0.125f * W_LOG2E, 0.125f, nullptr, st);
  const size_t bytes = (size_t)(2 * L.nwmax * 64 + 3 * L.nwmax) * 4;
  WIN_ATTR(attn_win_bwd_f32_kernel, WIN_F32_BWD_LDS);
  hipLaunchKernelGGL(attn_win_bwd_f32_kernel, dim3((unsigned)((L.G.nwin + 1) * B * H)), dim3(256), bytes, st,
                     (const float*)qkv, (const float*)dout, L.G, (int)N, (int)H, (float*)dqkv, 0.125f);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_attn_win_fwd_q2(const void* qkv, long B, long N, long gh, long gw, long wh, long ww, long H,
                                    long Dh, void* out, float* lse, const float* skip, void* stream) {
  WinLaunch L;
  if (int rc = win_check("ivit_attn_win_fwd_q2", B, N, gh, gw, wh, ww, H, Dh, L)) return rc;
  if (B == 0) return 0;
  return win_fwd_bf16_any(L, qkv, B, N, H, out, lse, 1.0f, 1.0f, win_drop_skip(skip), ivit_stream(stream));
}

// With q' = q c2 in qkv: P = exp2(q'k - lse2); dQ = dS K / 8 (the gradient w.r.t. the unscaled q);
// dK = ln2 dS^T q' = dS^T q / 8.
extern "C" int ivit_attn_win_bwd_q2(const void* qkv, const void* out, const void* dout, const float* lse, long B, long N,
                                    long gh, long gw, long wh, long ww, long H, long Dh, void* dqkv,
                                    const float* skip, void* stream) {
  (void)out;
  (void)lse;
  WinLaunch L;
  if (int rc = win_check("ivit_attn_win_bwd_q2", B, N, gh, gw, wh, ww, H, Dh, L)) return rc;
  if (B == 0) return 0;
  return win_bwd_bf16_any(L, qkv, dout, B, N, H, dqkv, 1.0f, W_LN2, win_drop_skip(skip), ivit_stream(stream));
}
