// Eval-path geometry (utils.py): anchors, axis/rotated IoU matrices, delta decode and
// torchvision-CPU-exact non-maximum suppression.
#include "geom.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

using namespace ivit;

namespace {

// utils.py:519-562: centres x=(off_y - (s*gy + s/2))*voxel, y=((s*gx + s/2) - off_x)*voxel;
// rows location-major, anchor-minor.
__global__ void anchors_kernel(int fh, int fw, int stride, const float* cfgs, int A, float voxel, float off_x,
                               float off_y, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)fh * fw * A) return;
  const int a = (int)(i % A);
  const long loc = i / A;
  const int gy = (int)(loc / fw), gx = (int)(loc % fw);
  const float px = (float)(gx * stride) + (float)stride / 2.0f;
  const float py = (float)(gy * stride) + (float)stride / 2.0f;
  out[i * 5 + 0] = (off_y - py) * voxel;
  out[i * 5 + 1] = (px - off_x) * voxel;
  out[i * 5 + 2] = cfgs[a * 3 + 0];
  out[i * 5 + 3] = cfgs[a * 3 + 1];
  out[i * 5 + 4] = cfgs[a * 3 + 2];
}

__global__ void iou_matrix_kernel(const float* b1, long n1, const float* b2, long n2, float* out, int rotated) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1 * n2) return;
  const long r = i / n2, c = i - r * n2;
  out[i] = rotated ? rotated_iou(b1 + r * 5, b2 + c * 5) : axis_iou(b1 + r * 5, b2 + c * 5);
}

// utils.py:227-257
IVIT_DEV void decode_one(const float* d, const float* a, float* o) {
  o[0] = d[0] * a[2] + a[0];
  o[1] = d[1] * a[3] + a[1];
  o[2] = expf(d[2]) * a[2];
  o[3] = expf(d[3]) * a[3];
  const float yaw = a[4] + atan2f(d[4], d[5]);
  o[4] = atan2f(sinf(yaw), cosf(yaw));
}

__global__ void decode_kernel(const float* rel, const float* anchors, const long* idx, long n, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  decode_one(rel + i * 6, anchors + (idx ? idx[i] : i) * 5, out + i * 5);
}

// ---- NMS (torchvision CPU nms_kernel_impl): stable descending sort; f32 corners/areas/IoU;
//      suppress j if (double)IoU > thr.
//
// torchvision's test, bit for bit: (double)RN32(inter / u) > thr with u = (area_i + area_j) - inter in
// f32, i.e. RN32(inter / u) >= t, t the smallest float whose double exceeds thr. The IEEE division is
// a ~10-instruction VALU sequence, and with divergent lanes the whole wave waits for it (anchors
// overlap their neighbours, so most 64-lane iterations had some lane dividing). Instead
// q = inter * rcp(u) (relative error < 2^-22) decides every pair whose q lies outside
// [t - 8 ulp, t + 8 ulp] (a margin of ~2^-20); the rest, and u <= 0 / non-finite operands / a
// threshold that is negative or below the normal floats, take the exact division. Disjoint pairs
// (inter = 0) are decided before any of it.
struct NmsThr {
  double thr;
  float lo, hi;
  int fast;
};
NmsThr nms_thr(double thr) {
  NmsThr r{thr, 0.f, 0.f, 0};
  if (!(thr >= 1e-30) || !(thr < 1e30)) return r;
  float t = (float)thr;
  while ((double)t <= thr) t = nextafterf(t, INFINITY);
  float tp;
  while ((double)(tp = nextafterf(t, -INFINITY)) > thr) t = tp;  // the smallest float above thr
  float lo = t, hi = t;
  for (int k = 0; k < 8; ++k) {
    lo = nextafterf(lo, -INFINITY);
    hi = nextafterf(hi, INFINITY);
  }
  r.lo = lo;
  r.hi = hi;
  r.fast = 1;
  return r;
}
IVIT_DEV bool nms_suppresses(float ix1, float iy1, float ix2, float iy2, float ia, float4 c, float ca,
                             const NmsThr& th) {
  // raw v_max / v_min: fmaxf / fminf on LDS values made the compiler canonicalise each operand
  // first (one more instruction per use); the corners are never NaN for finite decoded boxes
  auto vmax = [](float a, float b) { float d; asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; };
  auto vmin = [](float a, float b) { float d; asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; };
  const float xx1 = vmax(ix1, c.x), yy1 = vmax(iy1, c.y);
  const float xx2 = vmin(ix2, c.z), yy2 = vmin(iy2, c.w);
  const float w = vmax(0.f, xx2 - xx1), h = vmax(0.f, yy2 - yy1);
  const float inter = w * h;
  // disjoint boxes (most pairs): inter = 0 gives 0 / u = +-0 or NaN, never above a threshold >= 0
  if (th.fast && !(inter > 0.f)) return false;
  const float u = (ia + ca) - inter;
  // u in [2^-126, 2^126): rcp(u) is a normal float too (at u >= 2^126 it would be subnormal, flushed
  // or imprecise, and q could land on the wrong side of the margin)
  if (th.fast && u >= 1.17549435e-38f && u < 0x1p126f && inter < INFINITY) {
    const float q = inter * __builtin_amdgcn_rcpf(u);
    if (q >= th.hi) return true;
    if (q <= th.lo) return false;
  }
  const float ovr = inter / u;
  return (double)ovr > th.thr;
}

// One 64-thread workgroup per (row block rb, chunk of NMS_CB column blocks >= rb): the rows' boxes
// stay in registers while the chunk's column blocks pass through LDS (corners as one float4, the
// area), each block's boxes loaded into registers one block ahead. A workgroup per (rb, cb) pair
// meant ~4 M one-wave workgroups per eval batch (half of them empty, below the diagonal).
constexpr int NMS_CB = 8;
IVIT_DEV void nms_mask_body(const float* __restrict__ sb, long n, int nw, const NmsThr& th,
                            unsigned long long* __restrict__ mask, int rb, int cb0) {
  __shared__ float4 cxy[2][64];
  __shared__ float car[2][64];
  const int t = threadIdx.x;
  const long i = (long)rb * 64 + t;
  const bool row_ok = i < n;
  float ix1 = 0.f, iy1 = 0.f, ix2 = 0.f, iy2 = 0.f, ia = 0.f;
  if (row_ok) {
    ix1 = sb[i * 5 + 0]; iy1 = sb[i * 5 + 1]; ix2 = sb[i * 5 + 2]; iy2 = sb[i * 5 + 3]; ia = sb[i * 5 + 4];
  }
  const int cbs = max(cb0, rb), cb1 = min(cb0 + NMS_CB, nw);
  float4 pxy = make_float4(0.f, 0.f, 0.f, 0.f);
  float pa = 0.f;
  auto fetch = [&](int cb) {
    const long cj = (long)cb * 64 + t;
    if (cj < n) {
      pxy = make_float4(sb[cj * 5 + 0], sb[cj * 5 + 1], sb[cj * 5 + 2], sb[cj * 5 + 3]);
      pa = sb[cj * 5 + 4];
    }
  };
  if (cbs < cb1) fetch(cbs);
  for (int cb = cbs; cb < cb1; ++cb) {
    const int buf = (cb - cbs) & 1;
    cxy[buf][t] = pxy;
    car[buf][t] = pa;
    if (cb + 1 < cb1) fetch(cb + 1);
    __syncthreads();  // one wave: publishes this block's boxes (the other buffer is the next one's)
    const int lim = (int)min((long)64, n - (long)cb * 64);
    // a wave-uniform loop; the diagonal block keeps only the bits of boxes after this one
    const unsigned long long keep_mask = cb == rb ? (t == 63 ? 0ull : ~0ull << (t + 1)) : ~0ull;
    unsigned long long bits = 0;
    if (lim == 64) {
      // a full block: 8 boxes per group with constant bit positions and LDS offsets (the rolled loop
      // spent ~8 of its ~18 VALU per pair on the 64-bit variable shift, the select and the address)
      for (int k0 = 0; k0 < 64; k0 += 8) {
        unsigned by = 0;
        float4 cc[8];  // the group's corners read together (one LDS wait per group, not per pair)
#pragma unroll
        for (int e = 0; e < 8; ++e) cc[e] = cxy[buf][k0 + e];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (nms_suppresses(ix1, iy1, ix2, iy2, ia, cc[e], car[buf][k0 + e], th)) by |= 1u << e;
        bits |= (unsigned long long)by << k0;
      }
    } else {
      for (int k = 0; k < lim; ++k)
        if (nms_suppresses(ix1, iy1, ix2, iy2, ia, cxy[buf][k], car[buf][k], th)) bits |= 1ull << k;
    }
    if (row_ok) mask[i * nw + cb] = bits & keep_mask;
  }
}

constexpr int NMS_MAXW = 2048;  // n <= 131072

// The greedy walk of torchvision's nms over the suppression mask, one workgroup per sample. Column
// block c (64 sorted boxes) is settled by wave 0 on scalar registers: starting from removed[c], it
// visits only the boxes still standing (find-first-one of ~w above the last kept box, each kept
// box's diagonal word read by v_readlane) — one step per KEPT box. The update of the later words
// no longer sits between two columns' walks. Column c's kept rows reach
//   * words c+1 and c+2 through wave 0 itself, right after its walk of c: it loaded those two words
//     of all 64 rows of column c two columns ahead (with the diagonal word; two register sets), and
//     each kept lane ORs its two into removed[] (LDS atomics);
//   * words >= c+3 through waves 1-3: their loads are issued in iteration c+1 (up to 8 kept rows in
//     flight per word, held across the barrier) and OR-ed into removed[] in iteration c+2,
// so the walk of column w finds every contribution of columns < w in removed[w], and an iteration
// costs one walk or one load issue, not a walk plus a global round trip. Kept-row lists are
// triple-buffered (column j in slot j % 3).
IVIT_DEV void nms_scan_body(const unsigned long long* __restrict__ mask, long n, int nw, const int* __restrict__ order,
                             long* __restrict__ keep, long* __restrict__ count_out) {
  __shared__ unsigned long long removed[NMS_MAXW];
  __shared__ unsigned long long kept_s[3];
  __shared__ long cnt_s;
  __shared__ int kbit[3][64];
  if (n <= 0) {  // an empty sample, settled before ld_row clamps a row index to n - 1 = -1
    if (threadIdx.x == 0) *count_out = 0;
    return;
  }
  for (int w = threadIdx.x; w < nw; w += 256) removed[w] = 0ull;
  if (threadIdx.x == 0) cnt_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool w0 = threadIdx.x < 64;
  const int t = threadIdx.x - 64;  // bulk thread index (waves 1-3)
  // wave 0: column c's diagonal word, its two next words and the row's sorted index (lane = row),
  // four loads issued as inline asm so that the compiler's wait pass does not retire them early
  // (it cannot count them across the walk's loop and waited vmcnt(0), i.e. for the other set too);
  // rows / words past the end read clamped addresses, whose values no kept lane ever uses
  auto ld_row = [&](int c, unsigned long long& dg, unsigned long long& n1, unsigned long long& n2, int& od) {
    const int cc = min(c, nw - 1);
    const long row = min((long)cc * 64 + lane, n - 1);
    const unsigned long long* mr = mask + row * nw;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dg) : "v"(mr + cc) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(n1) : "v"(mr + min(cc + 1, nw - 1)) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(n2) : "v"(mr + min(cc + 2, nw - 1)) : "memory");
    asm volatile("global_load_dword %0, %1, off" : "=v"(od) : "v"(order + row) : "memory");
  };
  // two register sets, A for even and B for odd columns: a set is reloaded (two columns ahead)
  // right after its column's walk, so each column's words are in flight for a whole iteration
  // (rotating one set through copies would make every copy wait for its load)
  struct Row { unsigned long long dg, n1, n2; int od; };
  Row ra{0ull, 0ull, 0ull, 0}, rb{0ull, 0ull, 0ull, 0};
  if (w0) {
    ld_row(0, ra.dg, ra.n1, ra.n2, ra.od);
    ld_row(1, rb.dg, rb.n1, rb.n2, rb.od);
  }
  // bulk: the held words of column c-1's kept rows (<= 8 per word), two words per thread
  unsigned long long held[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) held[i][q] = 0ull;
  auto iter = [&](int c, Row& r) {
    if (w0) {
      // this set's four loads retired: at most the other set's four (issued after them) remain,
      // or those and the previous column's keep[] store
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      asm volatile("" : "+v"(r.dg), "+v"(r.n1), "+v"(r.n2), "+v"(r.od));
      const unsigned dlo = (unsigned)r.dg, dhi = (unsigned)(r.dg >> 32);
      const unsigned long long r0 = removed[c];
      unsigned long long w =
          ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(r0 >> 32)) << 32) |
          (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)r0);
      unsigned long long kept = 0ull;
      const int lim = (int)min((long)64, n - (long)c * 64);
      // (the walk over all 64 bits took 2-3 x as long: scan 1332 -> 859 us per eval step)
      const unsigned long long valid = lim == 64 ? ~0ull : (1ull << lim) - 1ull;
      unsigned long long cand = ~w & valid;
      while (cand) {
        const int i = __builtin_ctzll(cand);
        kept |= 1ull << i;
        w |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, i) << 32) |
             (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, i);
        cand = ~w & valid & ((~0ull << i) << 1);
      }
      const long base = cnt_s;
      if ((kept >> lane) & 1ull) {
        const int rk = __popcll(lane ? (kept & ((1ull << lane) - 1ull)) : 0ull);
        keep[base + rk] = r.od;
        kbit[c % 3][rk] = lane;
        if (c + 1 < nw) atomicOr(&removed[c + 1], r.n1);
        if (c + 2 < nw) atomicOr(&removed[c + 2], r.n2);
      }
      if (lane == 0) {
        kept_s[c % 3] = kept;
        cnt_s = base + __popcll(kept);
      }
      ld_row(c + 2, r.dg, r.n1, r.n2, r.od);
    } else {
      if (c >= 2) {  // apply column c-2's held words (words >= c+1)
        const int j = c - 2, K = __popcll(kept_s[j % 3]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int wc = j + 3 + t + 192 * i;
          if (wc < nw) {
            unsigned long long acc = 0ull;
#pragma unroll
            for (int q = 0; q < 8; ++q) acc |= held[i][q];
            for (int q = 8; q < K; ++q) acc |= mask[((long)j * 64 + kbit[j % 3][q]) * nw + wc];  // > 8 kept
            if (acc) atomicOr(&removed[wc], acc);
          }
        }
        for (int wc = j + 3 + 384 + t; wc < nw; wc += 192) {  // past the held words (n > 24 700)
          unsigned long long acc = 0ull;
          for (int q = 0; q < K; ++q) acc |= mask[((long)j * 64 + kbit[j % 3][q]) * nw + wc];
          if (acc) atomicOr(&removed[wc], acc);
        }
      }
      if (c >= 1) {  // issue column c-1's loads (words >= c+2)
        const int j = c - 1, K = __popcll(kept_s[j % 3]);
        long rbo[8];  // the kept rows' mask-row offsets, read from LDS before any load is issued
#pragma unroll
        for (int q = 0; q < 8; ++q) rbo[q] = ((long)j * 64 + kbit[j % 3][q]) * nw;  // q >= K: unused
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int wc = j + 3 + t + 192 * i;
#pragma unroll
          for (int q = 0; q < 8; ++q) held[i][q] = wc < nw && q < K ? mask[rbo[q] + wc] : 0ull;
        }
      }
    }
    __syncthreads();
  };
  for (int c = 0; c < nw; c += 2) {
    iter(c, ra);
    if (c + 1 < nw) iter(c + 1, rb);
  }
  if (threadIdx.x == 0) *count_out = cnt_s;
}

// ---- the NMS pipeline (sort, suppression mask, greedy walk) over a batch of samples, and the
// fused eval post-processing ---------------------------------------------------------------------
// Sample s owns rows lo(s) .. lo(s) + n(s) - 1 of every per-row array and the mask words mo(s) ..:
// host prefix offsets (seg [S+1], mask_off [S]: ivit_nms_batched), or a fixed capacity per sample
// with the row counts on the device (ivit_eval_post: nothing is read back before the NMS), or
// with every sample full (ivit_nms: one sample of row_stride rows, known on the host).
struct SegView {
  const long* seg;   // [S+1] row offsets, or null
  const long* moff;  // [S] mask word offsets (with seg)
  const int* cnt;    // [S] rows per sample (without seg); null: row_stride rows in every sample
  long row_stride, mask_stride;
  IVIT_DEV long lo(int s) const { return seg ? seg[s] : (long)s * row_stride; }
  IVIT_DEV long n(int s) const { return seg ? seg[s + 1] - seg[s] : cnt ? (long)cnt[s] : row_stride; }
  IVIT_DEV long mo(int s) const { return seg ? moff[s] : (long)s * mask_stride; }
};

// One sample per workgroup of PS_T threads (16 waves) for the selection and the score sort.
constexpr int PS_T = 1024;
constexpr int PS_D = 16;  // radix digits: 4 key bits per pass

// Ascending order of the key = torch's stable descending sort of the score: the IEEE order made
// unsigned, inverted; s + 0.0f makes -0 tie with +0 as torch's comparison sort does.
IVIT_DEV unsigned desc_key(float s) {
  const unsigned u = __float_as_uint(s + 0.0f);
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}

// Exclusive prefix of v over the workgroup in thread order; the total goes to wsum[16].
// wsum: 17 LDS words. The caller separates two calls by a barrier.
IVIT_DEV unsigned block_excl_scan(unsigned v, unsigned* wsum) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  if (wid == 0) {
    const unsigned w = lane < PS_T / 64 ? wsum[lane] : 0u;
    unsigned z = w;
#pragma unroll
    for (int o = 1; o < PS_T / 64; o <<= 1) {
      const unsigned y = __shfl_up(z, o, 64);
      if (lane >= o) z += y;
    }
    if (lane < PS_T / 64) wsum[lane] = z - w;
    if (lane == PS_T / 64 - 1) wsum[16] = z;
  }
  __syncthreads();
  return wsum[wid] + x - v;
}

// Stable LSD radix sort of n (key, value) pairs by ascending key, by one workgroup. Thread t owns
// the contiguous chunk [t*I, t*I + I), I = ceil(n / PS_T): it counts its chunk's digits into its
// own histogram column (hist[d * PS_T + t], no atomics), the digit-major exclusive scan of the
// columns gives every (digit, thread) its first slot, and the thread scatters its chunk in order —
// so equal digits keep their order and the sort is stable. Thread t scans entries 16t .. 16t + 15,
// which all belong to digit t / 64: wave d's sum is digit d's total, and a pass in which one digit
// holds all n keys moves nothing and is skipped (the scores of one eval sample share their top
// bits). Keys / values ping-pong between (k0, v0) and (k1, v1), global scratch that stays in L2;
// returns which pair holds the result. n < 2^31.
IVIT_DEV int block_radix_sort(unsigned* k0, int* v0, unsigned* k1, int* v1, int n, unsigned* hist, unsigned* wsum,
                              int* skip) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int I = (n + PS_T - 1) / PS_T;
  const int b0 = min(t * I, n), b1 = min(b0 + I, n);
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 4) {
    const unsigned* ki = cur ? k1 : k0;
    const int* vi = cur ? v1 : v0;
    unsigned* ko = cur ? k0 : k1;
    int* vo = cur ? v0 : v1;
#pragma unroll
    for (int d = 0; d < PS_D; ++d) hist[d * PS_T + t] = 0u;
    if (t == 0) *skip = 0;
    // the chunk in groups of 8 keys, each group's loads issued together (one L2 latency per group,
    // not per key: the LDS counter updates after them are a dependent chain the compiler cannot
    // overlap with the next key's load)
    for (int g0 = b0; g0 < b1; g0 += 8) {
      unsigned kr[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) kr[e] = g0 + e < b1 ? ki[g0 + e] : 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (g0 + e < b1) ++hist[((kr[e] >> shift) & 15u) * PS_T + t];
    }
    __syncthreads();
    unsigned c[PS_D], run = 0;
#pragma unroll
    for (int j = 0; j < PS_D; ++j) {
      c[j] = hist[t * PS_D + j];
      run += c[j];
    }
    unsigned x = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    if (wid == 0) {
      const unsigned w = lane < PS_D ? wsum[lane] : 0u;
      unsigned z = w;
#pragma unroll
      for (int o = 1; o < PS_D; o <<= 1) {
        const unsigned y = __shfl_up(z, o, 64);
        if (lane >= o) z += y;
      }
      if (lane < PS_D) {
        wsum[lane] = z - w;
        if (w == (unsigned)n) *skip = 1;
      }
    }
    __syncthreads();
    unsigned off = wsum[wid] + x - run;
#pragma unroll
    for (int j = 0; j < PS_D; ++j) {
      hist[t * PS_D + j] = off;
      off += c[j];
    }
    __syncthreads();
    if (!*skip) {
      for (int g0 = b0; g0 < b1; g0 += 8) {
        unsigned kr[8];
        int vr[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          kr[e] = g0 + e < b1 ? ki[g0 + e] : 0u;
          vr[e] = g0 + e < b1 ? vi[g0 + e] : 0;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (g0 + e < b1) {
            const unsigned slot = ((kr[e] >> shift) & 15u) * PS_T + t;
            const unsigned p = hist[slot];
            hist[slot] = p + 1u;
            ko[p] = kr[e];
            vo[p] = vr[e];
          }
        }
      }
      cur ^= 1;
    }
    __syncthreads();
  }
  return cur;
}

// torchvision's nms input for sorted row p: corners of box[order[p]] and the area (utils.py:266-272)
IVIT_DEV void sorted_corners(const float* q, float* d) {
  const float x1 = q[0] - q[2] / 2.f, y1 = q[1] - q[3] / 2.f, x2 = q[0] + q[2] / 2.f, y2 = q[1] + q[3] / 2.f;
  d[0] = x1;
  d[1] = y1;
  d[2] = x2;
  d[3] = y2;
  d[4] = (x2 - x1) * (y2 - y1);
}

// ivit_nms, stage 1: the same order by counting, rank(i) = #{j : s_j > s_i or (s_j == s_i and
// j < i)} (== on floats: -0 ties with +0), then the sorted corner boxes. O(n^2) spread over
// n / 256 workgroups: at n = 64 the call takes 28 us against 41 us through the one-workgroup
// radix sort below (profiles/nms_unify_bench.json), and small n is what a single call is for.
__global__ void nms_rank_kernel(const float* __restrict__ s, long n, int* __restrict__ order) {
  __shared__ float tile[256];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const float si = i < n ? s[i] : 0.f;
  long rank = 0;
  for (long j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    if (j0 + threadIdx.x < n) tile[threadIdx.x] = s[j0 + threadIdx.x];
    __syncthreads();
    const int lim = (int)min((long)256, n - j0);
    for (int k = 0; k < lim; ++k) {
      const float sj = tile[k];
      const long j = j0 + k;
      rank += (sj > si) || (sj == si && j < i);
    }
  }
  if (i < n) order[rank] = (int)i;
}

__global__ void nms_sorted_boxes_kernel(const float* __restrict__ b, const int* __restrict__ order, long n,
                                        float* __restrict__ sb) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) sorted_corners(b + (long)order[p] * 5, sb + p * 5);
}

// ivit_nms_batched, stage 1: one workgroup per sample — keys from the scores, the stable
// descending sort, the sorted corner boxes. k0/v0/k1/v1: [total] scratch.
__global__ __launch_bounds__(PS_T) void nms_sort_b_kernel(const float* __restrict__ b, const float* __restrict__ scores,
                                                          const long* __restrict__ seg, unsigned* k0, int* v0,
                                                          unsigned* k1, int* v1, int* __restrict__ order,
                                                          float* __restrict__ sb) {
  __shared__ unsigned hist[PS_D * PS_T];
  __shared__ unsigned wsum[20];
  __shared__ int skip;
  const int sm = blockIdx.x;
  const long o = seg[sm];
  const int n = (int)(seg[sm + 1] - o);
  for (int i = threadIdx.x; i < n; i += PS_T) {
    k0[o + i] = desc_key(scores[o + i]);
    v0[o + i] = i;
  }
  __syncthreads();
  const int r = block_radix_sort(k0 + o, v0 + o, k1 + o, v1 + o, n, hist, wsum, &skip);
  const int* ord = (r ? v1 : v0) + o;
  for (int p = threadIdx.x; p < n; p += PS_T) {
    const int q = ord[p];
    order[o + p] = q;
    sorted_corners(b + (o + q) * 5, sb + (o + p) * 5);
  }
}

// mask[p][w] bit k: sorted box 64w+k (> p) overlaps sorted box p with IoU > thr.
// grid (ceil(nwmax / NMS_CB), nwmax, samples)
__global__ __launch_bounds__(64) void nms_mask_b_kernel(const float* __restrict__ sb_all, SegView sv, NmsThr th,
                                                        unsigned long long* __restrict__ mask_all) {
  const int sm = blockIdx.z;
  const long o = sv.lo(sm), n = sv.n(sm);
  const int nw = (int)((n + 63) / 64);
  const int cb0 = blockIdx.x * NMS_CB, rb = blockIdx.y;
  if (cb0 >= nw || rb >= nw || cb0 + NMS_CB <= rb) return;
  nms_mask_body(sb_all + o * 5, n, nw, th, mask_all + sv.mo(sm), rb, cb0);
}

// grid (samples)
__global__ __launch_bounds__(256) void nms_scan_b_kernel(const unsigned long long* __restrict__ mask_all, SegView sv,
                                                         const int* __restrict__ order_all,
                                                         long* __restrict__ keep_all, long* __restrict__ count) {
  const int sm = blockIdx.x;
  const long o = sv.lo(sm), n = sv.n(sm);
  nms_scan_body(mask_all + sv.mo(sm), n, (int)((n + 63) / 64), order_all + o, keep_all + o, count + sm);
}

// ---- rotated NMS: the same sort, mask layout, walk and gather; only the stage that fills the
// mask differs. Sorted box p suppresses a later sorted box q iff
// (double)rotated_iou(box[p], box[q]) > thr, the higher-ranked box first (geom.h: the clip is not
// symmetric in its rounding), i.e. the decision equals ivit_rotated_iou(sorted, sorted)[p][q] > thr.
//
// Per sorted box, once (nms_rot_prep_kernel): the ccw f64 corners and the area that
// rotated_iou(Poly, A, Poly, A) takes (10 doubles: x[4], y[4], area, pad) and an f32 prefilter
// record (cx, cy, r, -; cos yaw, sin yaw, |w/2|, |l/2|): r is the half diagonal
// sqrt((w/2)^2 + (l/2)^2), rounded from f64 and inflated by NMS_ROT_SLACK. Every corner lies within the true half diagonal of the centre, so two boxes
// whose centres are further apart than r_p + r_q are disjoint. The f32 test d2 > (r_p + r_q)^2 has
// a relative rounding error below 2^-21 in d2 (one rounding in each difference, square, and the
// sum) and below 2^-22 in the right side; the slack of 1e-4 per radius exceeds both by two orders
// of magnitude and leaves a true gap of >= 9.9e-5 (r_p + r_q) between the rejected boxes. A box
// that passes the area guard (>= 1e-6) has r >= 7e-4, so the gap is >= 1.4e-7, while the f64 edge
// tests of the clip carry an error of ~1e-16 x (coordinate magnitude <= 1e6) = ~2e-10 of the same
// units: the clip of a rejected pair is empty and its IoU is exactly 0. Pairs that pass the circle
// test take the separating-axis test of the two rectangles in f32 (rot_sat_apart: the four edge
// normals; two rectangles are disjoint iff one of them separates them): with |d| <= r_p + r_q
// its projections carry an absolute rounding error below 1e-6 (r_p + r_q) (the cosines and sines
// are rounded from f64), and a pair is rejected only if an axis separates it by more than
// 1e-4 (r_p + r_q): the same true gap, the same argument (whichever box owns the axis: the
// clipped polygon's vertices stay that far outside one edge line of the clipping rectangle's
// half strip). On an eval sample in which every anchor passes it halves the exact tests
// (91 -> 46 per box). Boxes outside that range (|cx|, |cy| or r above 1e6) or with a non-finite
// field get r = NaN: every comparison with it is false and the pair falls through to the exact
// test. With thr < 0 (or NaN) the prefilter is off: an IoU of 0 exceeds a negative threshold.
constexpr float NMS_ROT_SLACK = 1.0001f;
constexpr float NMS_ROT_RANGE = 1e6f;

// grid (ceil(max n / 256), samples). boxes: the unsorted xywha rows of every sample; order: each
// sample's stable descending score order (local row indices).
__global__ __launch_bounds__(256) void nms_rot_prep_kernel(const float* __restrict__ boxes,
                                                           const int* __restrict__ order, SegView sv,
                                                           double* __restrict__ rp, float4* __restrict__ rc) {
  const int sm = blockIdx.y;
  const long o = sv.lo(sm), n = sv.n(sm);
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float* b = boxes + (o + order[o + p]) * 5;
  Poly P;
  const double A = rect_prepare(b, P);
  double* d = rp + (o + p) * 10;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d[i] = P.x[i];
    d[4 + i] = P.y[i];
  }
  d[8] = A;
  d[9] = 0.0;
  const double hw = (double)b[2] / 2.0, hl = (double)b[3] / 2.0;
  const float r = (float)sqrt(hw * hw + hl * hl) * NMS_ROT_SLACK;
  // written so that a NaN in any field fails it
  const bool sane = fabsf(b[0]) <= NMS_ROT_RANGE && fabsf(b[1]) <= NMS_ROT_RANGE && r <= NMS_ROT_RANGE &&
                    fabsf(b[4]) < INFINITY;
  rc[2 * (o + p)] = make_float4(b[0], b[1], sane ? r : __builtin_nanf(""), 0.f);
  rc[2 * (o + p) + 1] = make_float4((float)cos((double)b[4]), (float)sin((double)b[4]), fabsf(b[2] / 2.f),
                                    fabsf(b[3] / 2.f));
}

// a, b: (cos, sin, half width, half length) of two boxes whose centres differ by (dx, dy). True iff
// an edge normal of either separates them by more than slack. u = (cos, sin) is a box's width
// axis, v = (-sin, cos) its length axis; u_a.u_b = v_a.v_b = cos(ya - yb), u_a.v_b = -v_a.u_b =
// sin(ya - yb). A NaN anywhere makes every comparison false.
IVIT_DEV bool rot_sat_apart(float dx, float dy, float4 a, float4 b, float slack) {
  const float C = fabsf(a.x * b.x + a.y * b.y), S = fabsf(a.y * b.x - a.x * b.y);
  if (fabsf(dx * a.x + dy * a.y) > a.z + (b.z * C + b.w * S) + slack) return true;
  if (fabsf(dy * a.x - dx * a.y) > a.w + (b.z * S + b.w * C) + slack) return true;
  if (fabsf(dx * b.x + dy * b.y) > b.z + (a.z * C + a.w * S) + slack) return true;
  if (fabsf(dy * b.x - dx * b.y) > b.w + (a.z * S + a.w * C) + slack) return true;
  return false;
}

// One 64-thread workgroup per (row block rb, chunk of NMS_CB column blocks >= rb), as
// nms_mask_body. Almost every pair is disjoint and the exact clip is a few thousand f64
// operations, so a lane-per-row loop over the columns would run the clip on the few lanes whose
// pair overlaps while the rest of the wave waits. Instead the chunk is worked in passes of
// NMS_ROT_KC columns:
//   1. lane = row: the f32 prefilter against each of the pass's columns (their records in LDS);
//      the surviving (column block, row, column) triples are appended to an LDS list in ballot
//      order (the wave's count is uniform, no atomics);
//   2. lane = list entry: while the list holds 64 entries, 64 of them are taken from its front,
//      one exact rotated_iou per lane; a suppressing pair sets its bit in the (column block, row)
//      LDS word (atomicOr). What is left (< 64) stays in the list for the next pass, also across
//      column blocks, and only the chunk's last step runs with idle lanes;
//   3. lane = row, at the end of the chunk: the NMS_CB words go to the mask.
// A list per 64 x 32 columns that was emptied after every pass ran the exact phase with 26 % of
// its lanes holding a pair on an eval sample in which all 22 500 anchors pass (11-20 % on sparse
// samples): a pass seldom yields 64 pairs.
// LDS: list (64 left over + 64 x NMS_ROT_KC new entries of 15 bits) 1152 B + records 2 KiB +
// words 4 KiB = 7296 B per one-wave workgroup: 22 fit in a CU's 160 KiB, more than the 20 the
// kernel's 88 VGPRs allow (5 waves per SIMD), so LDS does not lower the occupancy. NMS_ROT_KC = 32
// would cap it at 4 waves per SIMD. The clip's polygons are indexed at run time and live in scratch, so the exact
// phase is latency-bound and wants the waves.
constexpr int NMS_ROT_KC = 8;
IVIT_DEV void nms_rot_mask_body(const double* __restrict__ rp, const float4* __restrict__ rc, long n, int nw,
                                double thr, int pre, unsigned long long* __restrict__ mask, int rb, int cb0) {
  __shared__ float4 ccol[64], ccol2[64];
  __shared__ unsigned short plist[64 + 64 * NMS_ROT_KC];
  __shared__ unsigned long long bits_s[NMS_CB][64];
  const int t = threadIdx.x;
  const long i = (long)rb * 64 + t;
  const bool row_ok = i < n;
  const float4 me = row_ok ? rc[2 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 me2 = row_ok ? rc[2 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned long long below = t ? (~0ull >> (64 - t)) : 0ull;  // the lanes before this one
  const int cbs = max(cb0, rb), cb1 = min(cb0 + NMS_CB, nw);
#pragma unroll
  for (int c = 0; c < NMS_CB; ++c) bits_s[c][t] = 0ull;
  // one exact test: list entry = (column block - cb0) << 12 | row << 6 | column
  auto exact = [&](int ent) {
    const int ci = ent >> 12, r = (ent >> 6) & 63, k = ent & 63;
    const double* a = rp + ((long)rb * 64 + r) * 10;
    const double* b = rp + ((long)(cb0 + ci) * 64 + k) * 10;
    Poly pa, pb;
    pa.n = 4;
    pb.n = 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pa.x[q] = a[q];
      pa.y[q] = a[4 + q];
      pb.x[q] = b[q];
      pb.y[q] = b[4 + q];
    }
    if ((double)rotated_iou(pa, a[8], pb, b[8]) > thr) atomicOr(&bits_s[ci][r], 1ull << k);
  };
  int cnt = 0;  // list length, wave-uniform, < 64 between passes
  for (int cb = cbs; cb < cb1; ++cb) {
    const long cj = (long)cb * 64 + t;
    __syncthreads();  // the previous block's records are no longer read
    if (cj < n) {
      ccol[t] = rc[2 * cj];
      ccol2[t] = rc[2 * cj + 1];
    }
    __syncthreads();
    const int lim = (int)min((long)64, n - (long)cb * 64);
    // the diagonal block tests (and keeps) only the boxes after this one
    const int kfirst = cb == rb ? t + 1 : 0;
    const int tag = ((cb - cb0) << 12) | (t << 6);
    for (int kc = 0; kc < lim; kc += NMS_ROT_KC) {
      const int k1 = min(kc + NMS_ROT_KC, lim);
      for (int k = kc; k < k1; ++k) {
        bool cand = row_ok && k >= kfirst;
        if (cand && pre) {
          const float4 c = ccol[k];
          const float dx = me.x - c.x, dy = me.y - c.y, R = me.z + c.z;
          // a NaN on either side: both tests are false, the pair stays
          if (dx * dx + dy * dy > R * R || rot_sat_apart(dx, dy, me2, ccol2[k], 1e-4f * R)) cand = false;
        }
        const unsigned long long bal = __ballot(cand);
        if (cand) plist[cnt + __popcll(bal & below)] = (unsigned short)(tag | k);
        cnt += __popcll(bal);
      }
      if (cnt < 64) continue;  // wave-uniform
      __syncthreads();
      const int full = cnt & ~63, rem = cnt - full;
      for (int e0 = 0; e0 < full; e0 += 64) exact(plist[e0 + t]);
      const int left = t < rem ? plist[full + t] : 0;
      __syncthreads();  // every entry has been read: the rest moves to the front
      if (t < rem) plist[t] = (unsigned short)left;
      cnt = rem;
    }
  }
  __syncthreads();
  if (t < cnt) exact(plist[t]);
  __syncthreads();
  for (int cb = cbs; cb < cb1; ++cb) {
    const unsigned long long keep_mask = cb == rb ? (t == 63 ? 0ull : ~0ull << (t + 1)) : ~0ull;
    if (row_ok) mask[i * nw + cb] = bits_s[cb - cb0][t] & keep_mask;
  }
}

// grid (ceil(nwmax / NMS_CB), nwmax, samples)
__global__ __launch_bounds__(64) void nms_rot_mask_b_kernel(const double* __restrict__ rp_all,
                                                            const float4* __restrict__ rc_all, SegView sv, double thr,
                                                            int pre, unsigned long long* __restrict__ mask_all) {
  const int sm = blockIdx.z;
  const long o = sv.lo(sm), n = sv.n(sm);
  const int nw = (int)((n + 63) / 64);
  const int cb0 = blockIdx.x * NMS_CB, rb = blockIdx.y;
  if (cb0 >= nw || rb >= nw || cb0 + NMS_CB <= rb) return;
  nms_rot_mask_body(rp_all + o * 10, rc_all + 2 * o, n, nw, thr, pre, mask_all + sv.mo(sm), rb, cb0);
}

// ---- eval post-processing (eval_vit.py:156-176) for a whole batch, capacity NA rows per sample.
struct PostWs {
  int* n;            // [S] rows passing the confidence threshold
  int* anchor;       // [S*NA] anchor index of compacted row p
  float* score;      // [S*NA]
  float* box;        // [S*NA*5] decoded (utils.py:227-257)
  unsigned *k0, *k1;  // sort scratch
  int *v0, *v1;
  int* order;        // [S*NA] stable descending score order (compacted-row indices)
  float* sb;         // [S*NA*5] sorted corners + area
  long* keep;        // [S*NA] kept compacted-row indices in score order
  unsigned long long* mask;
  double* rp;        // [S*NA*10] rotated only: nms_rot_prep_kernel's polygons
  float4* rc;        // [S*NA*2]  and prefilter records
};

// torch's f32 sigmoid on the GPU: 1 / (1 + exp(-x)), IEEE division (UnarySpecialOpsKernel.cu)
IVIT_DEV float torch_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// eval_vit.py:159-168 for sample blockIdx.x: scores = sigmoid(cls); where(score >= conf) in anchor
// order (a workgroup-wide exclusive scan of per-thread counts: thread t owns anchors
// [t*I, t*I + I)); the compacted scores, anchor indices and decoded boxes; then apply_nms's stable
// descending score order and its sorted corner boxes. NaN logits fail the threshold, as in torch.
__global__ __launch_bounds__(PS_T) void post_select_kernel(const float* __restrict__ cls, const float* __restrict__ rel,
                                                           const float* __restrict__ anchors, int NA, float conf,
                                                           PostWs w) {
  __shared__ unsigned hist[PS_D * PS_T];
  __shared__ unsigned wsum[20];
  __shared__ int skip;
  const int sm = blockIdx.x, t = threadIdx.x;
  const long base = (long)sm * NA;
  const float* c = cls + base;
  const float* r = rel + base * 6;
  const int I = (NA + PS_T - 1) / PS_T;
  const int a0 = min(t * I, NA), a1 = min(a0 + I, NA);
  unsigned np = 0;
  for (int g0 = a0; g0 < a1; g0 += 8) {  // the logits of 8 anchors loaded together
    float lr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) lr[e] = g0 + e < a1 ? c[g0 + e] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) np += g0 + e < a1 && torch_sigmoid(lr[e]) >= conf;
  }
  unsigned p = block_excl_scan(np, wsum);
  const int n = (int)wsum[16];
  for (int g0 = a0; g0 < a1; g0 += 8) {
    float lr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) lr[e] = g0 + e < a1 ? c[g0 + e] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int a = g0 + e;
      const float s = torch_sigmoid(lr[e]);
      if (a < a1 && s >= conf) {
        const long q = base + p;
        w.anchor[q] = a;
        w.score[q] = s;
        w.k0[q] = desc_key(s);
        w.v0[q] = (int)p;
        decode_one(r + (long)a * 6, anchors + (long)a * 5, w.box + q * 5);
        ++p;
      }
    }
  }
  if (t == 0) w.n[sm] = n;
  __syncthreads();
  const int res = block_radix_sort(w.k0 + base, w.v0 + base, w.k1 + base, w.v1 + base, n, hist, wsum, &skip);
  const int* ord = (res ? w.v1 : w.v0) + base;
  for (int i = t; i < n; i += PS_T) {
    const int q = ord[i];
    w.order[base + i] = q;
    sorted_corners(w.box + (base + q) * 5, w.sb + (base + i) * 5);
  }
}

// eval_vit.py:172-175: kept row j of sample s (blockIdx.y) -> its score, decoded box and the
// argmax intention of its anchor (first maximum; a NaN is the maximum, the first NaN wins — torch's
// argmax), packed at s * NA + j.
__global__ void post_gather_kernel(const long* __restrict__ kcnt, const float* __restrict__ intent, int NA, int K,
                                   PostWs w, float* __restrict__ out_score, float* __restrict__ out_box,
                                   long* __restrict__ out_int) {
  const int sm = blockIdx.y;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= kcnt[sm]) return;
  const long base = (long)sm * NA, k = base + w.keep[base + j], q = base + j;
  out_score[q] = w.score[k];
#pragma unroll
  for (int e = 0; e < 5; ++e) out_box[q * 5 + e] = w.box[k * 5 + e];
  const float* lg = intent + (base + w.anchor[k]) * K;
  int best = 0;
  float bv = lg[0];
  for (int e = 1; e < K; ++e) {
    const float v = lg[e];
    if (bv == bv && (v > bv || v != v)) {
      bv = v;
      best = e;
    }
  }
  out_int[q] = best;
}

}  // namespace

extern "C" int ivit_generate_anchors(long bev_h, long bev_w, long stride, const float* cfgs, long A, float voxel,
                                     float off_x, float off_y, float* out, void* stream) {
  IVIT_CHECK_ARG(stride > 0 && bev_h >= 0 && bev_w >= 0 && A >= 0, "ivit_generate_anchors: bad sizes (stride %ld)",
                 stride);
  const int fh = (int)(bev_h / stride), fw = (int)(bev_w / stride);
  const long n = (long)fh * fw * A;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(anchors_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), fh, fw, (int)stride,
                     cfgs, (int)A, voxel, off_x, off_y, out);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_axis_iou(const float* b1, long n1, const float* b2, long n2, float* out, void* stream) {
  if (n1 * n2 <= 0) return 0;
  hipLaunchKernelGGL(iou_matrix_kernel, dim3(ivit_cdiv(n1 * n2, 256)), dim3(256), 0, ivit_stream(stream), b1, n1, b2,
                     n2, out, 0);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_rotated_iou(const float* b1, long n1, const float* b2, long n2, float* out, void* stream) {
  if (n1 * n2 <= 0) return 0;
  hipLaunchKernelGGL(iou_matrix_kernel, dim3(ivit_cdiv(n1 * n2, 128)), dim3(128), 0, ivit_stream(stream), b1, n1, b2,
                     n2, out, 1);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_decode_boxes(const float* rel, const float* anchors, const long* idx, long n, float* out,
                                 void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(decode_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), rel, anchors, idx, n,
                     out);
  IVIT_LAUNCH_CHECK();
  return 0;
}

// ---- NMS entries. Every one of them runs sort -> suppression mask -> greedy walk; the five
// entries differ in who sorts (nms_rank_kernel for one sample, nms_sort_b_kernel for a batch,
// post_select_kernel after its selection), in the SegView, and in the suppression test.
namespace {
long al16(long b) { return (b + 15) / 16 * 16; }

// IVIT_LAUNCH_CHECK for the shared implementations: the message names the entry that was called
int launch_status(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) ivit_set_error("%s: %s", name, hipGetErrorString(e));
  return (int)e;
}

// The stages after the sort, for samples whose largest row count is max_n: [the rotated test's
// per-box polygons and prefilter records ->] the suppression mask -> the greedy walk.
// boxes: the unsorted xywha rows and rp / rc: the per-box records (rotated only); sb: the sorted
// corner rows (axis only).
void nms_mask_and_scan(const float* boxes, const int* order, const float* sb, double* rp, float4* rc,
                       unsigned long long* mask, const SegView& sv, long samples, long max_n, double thr, bool rotated,
                       long* keep, long* count, hipStream_t st) {
  const int nwmax = (int)((max_n + 63) / 64);
  const dim3 mask_grid(ivit_cdiv(nwmax, NMS_CB), nwmax, samples);
  if (rotated) {
    hipLaunchKernelGGL(nms_rot_prep_kernel, dim3(ivit_cdiv(max_n, 256), samples), dim3(256), 0, st, boxes, order, sv,
                       rp, rc);
    hipLaunchKernelGGL(nms_rot_mask_b_kernel, mask_grid, dim3(64), 0, st, rp, rc, sv, thr, thr >= 0.0 ? 1 : 0, mask);
  } else {
    hipLaunchKernelGGL(nms_mask_b_kernel, mask_grid, dim3(64), 0, st, sb, sv, nms_thr(thr), mask);
  }
  hipLaunchKernelGGL(nms_scan_b_kernel, dim3(samples), dim3(256), 0, st, mask, sv, order, keep, count);
}

// The workspace of ivit_nms_batched / ivit_nms_rotated_batched, regions in this order,
// each rounded up to 16 bytes, after a base rounded up to 16 (bytes includes 64 of slack for it).
// The rotated form appends the polygons (80 B per row) and the prefilter records (32 B per row);
// its sort stage is the shared one and still writes the corner rows.
struct BatchWs {
  int* order;                // [total]
  float* sb;                 // [total*5]
  unsigned long long* mask;  // [mask_words]
  unsigned *k0, *k1;         // [total] sort scratch
  int *v0, *v1;
  double* rp;                // [total*10], rotated only
  float4* rc;                // [total*2], rotated only
  long bytes;
};
BatchWs batch_ws(void* work, long total, long mask_words, bool rotated) {
  const uintptr_t base = ((uintptr_t)work + 15) & ~(uintptr_t)15;
  long off = 0;
  auto take = [&](long bytes) {
    void* p = (void*)(base + off);
    off += al16(bytes);
    return p;
  };
  BatchWs w{};
  w.order = (int*)take(4 * total);
  w.sb = (float*)take(20 * total);
  w.mask = (unsigned long long*)take(8 * mask_words);
  w.k0 = (unsigned*)take(4 * total);
  w.k1 = (unsigned*)take(4 * total);
  w.v0 = (int*)take(4 * total);
  w.v1 = (int*)take(4 * total);
  if (rotated) {
    w.rp = (double*)take(80 * total);
    w.rc = (float4*)take(32 * total);
  }
  w.bytes = off + 64;
  return w;
}
long batch_ws_bytes(long n_samples, long total, long mask_words, bool rotated) {
  if (n_samples <= 0 || total <= 0) return 64;
  return batch_ws(nullptr, total, mask_words, rotated).bytes;
}

// Batched torchvision-CPU-exact NMS (eval_vit.py:170 per sample, all samples in one launch per
// stage). keep[lo(s) ..] receives sample s's kept LOCAL indices in score order, count[s] their
// number. The score order is a stable descending sort (nms_sort_b_kernel: one workgroup per
// sample; ties keep the row order, as torch's stable sort). With rotated, sorted box p suppresses
// a later q iff (double)rotated_iou(p, q) > iou_thr.
int nms_batched_impl(const char* name, bool rotated, const float* boxes_xywha, const float* scores, const long* seg,
                     const long* mask_off, long n_samples, long total, long max_n, long mask_words, double iou_thr,
                     long* keep, long* count, void* work, long work_bytes, void* stream) {
  IVIT_CHECK_ARG(max_n <= 64L * NMS_MAXW, "%s: n=%ld exceeds %d", name, max_n, 64 * NMS_MAXW);
  IVIT_CHECK_ARG(n_samples < 65536 && total < (1L << 31), "%s: too many samples / rows (%ld, %ld)", name, n_samples,
                 total);
  IVIT_CHECK_ARG(work_bytes >= batch_ws_bytes(n_samples, total, mask_words, rotated), "%s: workspace too small", name);
  hipStream_t st = ivit_stream(stream);
  if (n_samples <= 0) return 0;
  if (max_n <= 0 || total <= 0) {
    (void)hipMemsetAsync(count, 0, sizeof(long) * n_samples, st);
    return launch_status(name);
  }
  const BatchWs w = batch_ws(work, total, mask_words, rotated);
  const SegView sv{seg, mask_off, nullptr, 0, 0};
  hipLaunchKernelGGL(nms_sort_b_kernel, dim3(n_samples), dim3(PS_T), 0, st, boxes_xywha, scores, seg, w.k0, w.v0, w.k1,
                     w.v1, w.order, w.sb);
  nms_mask_and_scan(boxes_xywha, w.order, w.sb, w.rp, w.rc, w.mask, sv, n_samples, max_n, iou_thr, rotated, keep,
                    count, st);
  return launch_status(name);
}
}  // namespace

// One sample of n rows, n known on the host: its own sort stage, which needs no scratch, then the
// shared stages with a one-sample SegView. It uses the first three regions of BatchWs; their
// rounding (base <= 15, order and sb <= 12 each) fits the 64 bytes of slack in its workspace.
extern "C" long ivit_nms_workspace(long n) {
  const long nw = (n + 63) / 64;
  return n * 4 + n * 5 * 4 + n * nw * 8 + 64;
}

extern "C" int ivit_nms(const float* boxes_xywha, const float* scores, long n, double iou_thr, long* keep, long* count,
                        void* work, long work_bytes, void* stream) {
  IVIT_CHECK_ARG(n <= 64L * NMS_MAXW, "ivit_nms: n=%ld exceeds %d", n, 64 * NMS_MAXW);
  IVIT_CHECK_ARG(work_bytes >= ivit_nms_workspace(n), "ivit_nms: workspace too small");
  hipStream_t st = ivit_stream(stream);
  if (n <= 0) {
    (void)hipMemsetAsync(count, 0, sizeof(long), st);
    IVIT_LAUNCH_CHECK();
    return 0;
  }
  const BatchWs w = batch_ws(work, n, n * ((n + 63) / 64), false);
  hipLaunchKernelGGL(nms_rank_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, st, scores, n, w.order);
  hipLaunchKernelGGL(nms_sorted_boxes_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, st, boxes_xywha, w.order, n, w.sb);
  nms_mask_and_scan(boxes_xywha, w.order, w.sb, nullptr, nullptr, w.mask, SegView{nullptr, nullptr, nullptr, n, 0}, 1,
                    n, iou_thr, false, keep, count, st);
  IVIT_LAUNCH_CHECK();
  return 0;
}

// seg: [S+1] int64 row offsets (device); mask_off: [S] int64 word offsets of each sample's
// [n_s, ceil(n_s/64)] suppression mask (device).
extern "C" long ivit_nms_batched_workspace(long n_samples, long total, long mask_words) {
  return batch_ws_bytes(n_samples, total, mask_words, false);
}

extern "C" int ivit_nms_batched(const float* boxes_xywha, const float* scores, const long* seg, const long* mask_off,
                                long n_samples, long total, long max_n, long mask_words, double iou_thr, long* keep,
                                long* count, void* work, long work_bytes, void* stream) {
  return nms_batched_impl("ivit_nms_batched", false, boxes_xywha, scores, seg, mask_off, n_samples, total, max_n,
                          mask_words, iou_thr, keep, count, work, work_bytes, stream);
}

extern "C" long ivit_nms_rotated_batched_workspace(long n_samples, long total, long mask_words) {
  return batch_ws_bytes(n_samples, total, mask_words, true);
}

extern "C" int ivit_nms_rotated_batched(const float* boxes_xywha, const float* scores, const long* seg,
                                        const long* mask_off, long n_samples, long total, long max_n, long mask_words,
                                        double iou_thr, long* keep, long* count, void* work, long work_bytes,
                                        void* stream) {
  return nms_batched_impl("ivit_nms_rotated_batched", true, boxes_xywha, scores, seg, mask_off, n_samples, total,
                          max_n, mask_words, iou_thr, keep, count, work, work_bytes, stream);
}

// Eval post-processing for a batch (eval_vit.py:156-176): four launches (five with the rotated
// test: the per-box polygons are one more), no host round trip.
namespace {
// The workspace: one region per PostWs member in the member order, then (rotated only) rp and rc,
// each rounded up to 16 bytes, plus 16 of slack for rounding the base up. The mask is reserved
// for the worst case, every anchor of every sample passing.
constexpr int POST_REGIONS = 14;
struct PostLayout {
  long bytes;
  long off[POST_REGIONS];
  int regions;  // 12, or 14 with rotated
};
PostLayout post_layout(long B, long NA, bool rotated) {
  const long R = B * NA, nw = (NA + 63) / 64;
  const long sz[POST_REGIONS] = {4 * B, 4 * R, 4 * R, 20 * R, 4 * R,      4 * R,  4 * R,
                                 4 * R, 4 * R, 20 * R, 8 * R, 8 * R * nw, 80 * R, 32 * R};
  PostLayout L{0, {}, rotated ? 14 : 12};
  for (int i = 0; i < L.regions; ++i) {
    L.off[i] = L.bytes;
    L.bytes += al16(sz[i]);
  }
  L.bytes += 16;  // alignment slack
  return L;
}
long post_ws_bytes(long B, long NA, bool rotated) {
  if (B <= 0 || NA <= 0) return 64;
  return post_layout(B, NA, rotated).bytes;
}
PostWs post_ws(void* work, long B, long NA, bool rotated) {
  const PostLayout L = post_layout(B, NA, rotated);
  char* base = (char*)(((uintptr_t)work + 15) & ~(uintptr_t)15);
  auto at = [&](int i) -> void* { return i < L.regions ? base + L.off[i] : nullptr; };
  PostWs w;
  w.n = (int*)at(0);
  w.anchor = (int*)at(1);
  w.score = (float*)at(2);
  w.box = (float*)at(3);
  w.k0 = (unsigned*)at(4);
  w.k1 = (unsigned*)at(5);
  w.v0 = (int*)at(6);
  w.v1 = (int*)at(7);
  w.order = (int*)at(8);
  w.sb = (float*)at(9);
  w.keep = (long*)at(10);
  w.mask = (unsigned long long*)at(11);
  w.rp = (double*)at(12);
  w.rc = (float4*)at(13);
  return w;
}

int eval_post_impl(const char* name, bool rotated, const float* cls, const float* box_rel, const float* intent,
                   const float* anchors, long B, long NA, long K, float conf_thr, double iou_thr, float* out_scores,
                   float* out_boxes, long* out_intent, long* out_count, void* work, long work_bytes, void* stream) {
  IVIT_CHECK_ARG(B >= 0 && B < 65536 && NA >= 0 && K >= 1, "%s: bad sizes (B %ld, NA %ld, K %ld)", name, B, NA, K);
  IVIT_CHECK_ARG(NA <= 64L * NMS_MAXW, "%s: NA=%ld exceeds %d", name, NA, 64 * NMS_MAXW);
  IVIT_CHECK_ARG(work_bytes >= post_ws_bytes(B, NA, rotated), "%s: workspace too small", name);
  hipStream_t st = ivit_stream(stream);
  if (B == 0) return 0;
  if (NA == 0) {
    (void)hipMemsetAsync(out_count, 0, sizeof(long) * B, st);
    return launch_status(name);
  }
  const PostWs w = post_ws(work, B, NA, rotated);
  const SegView sv{nullptr, nullptr, w.n, NA, NA * ((NA + 63) / 64)};
  hipLaunchKernelGGL(post_select_kernel, dim3(B), dim3(PS_T), 0, st, cls, box_rel, anchors, (int)NA, conf_thr, w);
  nms_mask_and_scan(w.box, w.order, w.sb, w.rp, w.rc, w.mask, sv, B, NA, iou_thr, rotated, w.keep, out_count, st);
  hipLaunchKernelGGL(post_gather_kernel, dim3(ivit_cdiv(NA, 256), B), dim3(256), 0, st, out_count, intent, (int)NA,
                     (int)K, w, out_scores, out_boxes, out_intent);
  return launch_status(name);
}
}  // namespace

extern "C" long ivit_eval_post_workspace(long B, long NA) { return post_ws_bytes(B, NA, false); }

extern "C" int ivit_eval_post(const float* cls, const float* box_rel, const float* intent, const float* anchors, long B,
                              long NA, long K, float conf_thr, double iou_thr, float* out_scores, float* out_boxes,
                              long* out_intent, long* out_count, void* work, long work_bytes, void* stream) {
  return eval_post_impl("ivit_eval_post", false, cls, box_rel, intent, anchors, B, NA, K, conf_thr, iou_thr,
                        out_scores, out_boxes, out_intent, out_count, work, work_bytes, stream);
}

extern "C" long ivit_eval_post_rotated_workspace(long B, long NA) { return post_ws_bytes(B, NA, true); }

extern "C" int ivit_eval_post_rotated(const float* cls, const float* box_rel, const float* intent, const float* anchors,
                                      long B, long NA, long K, float conf_thr, double iou_thr, float* out_scores,
                                      float* out_boxes, long* out_intent, long* out_count, void* work, long work_bytes,
                                      void* stream) {
  return eval_post_impl("ivit_eval_post_rotated", true, cls, box_rel, intent, anchors, B, NA, K, conf_thr, iou_thr,
                        out_scores, out_boxes, out_intent, out_count, work, work_bytes, stream);
}


// ---- weighted box fusion behind the NMS stages (ivit_nms_fuse_batched, ivit_eval_post_tta) -------
// The sort, the suppression mask and the greedy walk are the shared ones, unchanged. When the walk
// ends the full upper-triangular mask is still in memory: row p of a kept box (a leader) names
// every later sorted box it overlaps. A suppressed box q was removed by the FIRST leader in score
// order whose row has bit q (the walk ORs the rows of the kept boxes in that order), so
//   fuse_rank_kernel   rank[] = the inverse of order[] (a leader's sorted position), owner[] = none;
//   fuse_owner_kernel  one wave per leader j over its mask row: atomicMin(owner[q], j) for every
//                      set bit (an integer minimum: the arrival order cannot change it);
//   fuse_cluster_kernel one wave per leader j over the same row, keeping the bits q whose owner is
//                      j: the score-weighted f64 sums of the members aligned to the leader, the
//                      intention vote, the per-view score maxima, the member count. Lane l adds the
//                      members of words first + l, first + l + 64, ... in ascending bit order
//                      (lane 0 starts with the leader itself), then the 64 partial sums are added in
//                      a fixed xor butterfly (a + b = b + a bitwise, so every lane holds the same
//                      sum): the order is a function of the sample's own rows alone;
//   fuse_emit_kernel   one workgroup per sample: the stable descending sort of the fused scores
//                      (two views with fusion only; otherwise the keep order is that order
//                      already) and the packed output rows.
// Two leaders never share a bit (a kept box is not overlapped by an earlier kept box), so a
// leader's own entry is written by its own wave alone.
namespace {
struct FuseWs {
  const float* box;    // candidate rows, unsorted xywha
  const float* score;
  const int* intent;
  const int* views;    // per row, or null
  const int* split;    // [S] rows of view 0 (the rest are view 1), or null; views wins
  const int* order;
  const long* keep;
  const long* count;
  const unsigned long long* mask;
  int* rank;           // [rows] sorted position of local row r
  int* owner;          // [rows] by sorted position: the owning leader's place in the keep list
  float* tbox;         // [rows*5] per leader j (the corner rows' region: dead after the mask)
  float* tscore;       // [rows]
  int* tint;           // [rows]
  int* tmem;           // [rows]
  unsigned *k0, *k1;   // the sort scratch, dead after the first sort
  int *v0, *v1;
  int K, n_views, fuse;
};
constexpr int FUSE_NONE = 0x7fffffff;
constexpr int FUSE_MAXK = 32;
constexpr double FUSE_HALF_PI = 1.5707963267948966;
constexpr double FUSE_PI = 3.141592653589793;

IVIT_DEV int fuse_view(const FuseWs& f, int sm, long o, int r) {
  if (f.n_views < 2) return 0;
  if (f.views) return f.views[o + r] != 0;
  return f.split ? r >= f.split[sm] : 0;
}

// grid (ceil(max n / 256), samples)
__global__ __launch_bounds__(256) void fuse_rank_kernel(FuseWs f, SegView sv) {
  const int sm = blockIdx.y;
  const long o = sv.lo(sm), n = sv.n(sm);
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  f.rank[o + f.order[o + p]] = (int)p;
  f.owner[o + p] = FUSE_NONE;
}

// grid (x, samples), 4 waves per workgroup, leaders strided over the sample's waves
__global__ __launch_bounds__(256) void fuse_owner_kernel(FuseWs f, SegView sv) {
  const int sm = blockIdx.y, lane = threadIdx.x & 63;
  const long o = sv.lo(sm), n = sv.n(sm);
  const int nw = (int)((n + 63) / 64);
  const long cnt = min(f.count[sm], n);
  const unsigned long long* mask = f.mask + sv.mo(sm);
  for (long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6); j < cnt; j += (long)gridDim.x * 4) {
    const int p = f.rank[o + f.keep[o + j]];
    if (lane == 0) atomicMin(&f.owner[o + p], (int)j);
    const unsigned long long* row = mask + (long)p * nw;
    for (int w = (p >> 6) + lane; w < nw; w += 64) {
      unsigned long long bits = row[w];
      while (bits) {
        const long q = (long)w * 64 + __builtin_ctzll(bits);
        bits &= bits - 1ull;
        if (q < n) atomicMin(&f.owner[o + q], (int)j);
      }
    }
  }
}

IVIT_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// grid (x, samples), one wave per workgroup, leaders strided over the sample's workgroups
__global__ __launch_bounds__(64) void fuse_cluster_kernel(FuseWs f, SegView sv) {
  __shared__ double vote[FUSE_MAXK][64];
  const int sm = blockIdx.y, lane = threadIdx.x;
  const long o = sv.lo(sm), n = sv.n(sm);
  const int nw = (int)((n + 63) / 64);
  const long cnt = min(f.count[sm], n);
  const unsigned long long* mask = f.mask + sv.mo(sm);
  for (long j = blockIdx.x; j < cnt; j += gridDim.x) {
    const int rp = (int)f.keep[o + j];
    const int p = f.rank[o + rp];
    const float* bp = f.box + (o + rp) * 5;
    const double ap = (double)bp[4];
    double S = 0.0, sx = 0.0, sy = 0.0, sw = 0.0, sl = 0.0, sd = 0.0;
    float m0 = -INFINITY, m1 = -INFINITY;
    int members = 0;
    if (f.fuse)
      for (int c = 0; c < f.K; ++c) vote[c][lane] = 0.0;
    auto member = [&](int q) {
      const int r = f.order[o + q];
      ++members;
      if (!f.fuse) return;
      const float* b = f.box + (o + r) * 5;
      const float sc = f.score[o + r];
      const double s = (double)sc;
      const double d = (double)b[4] - ap;
      const double k = rint(d / FUSE_HALF_PI);
      const double delta = d - k * FUSE_HALF_PI;
      const bool odd = ((long long)k) & 1;
      S += s;
      sx += s * (double)b[0];
      sy += s * (double)b[1];
      sw += s * (double)(odd ? b[3] : b[2]);
      sl += s * (double)(odd ? b[2] : b[3]);
      sd += s * delta;
      const int c = f.intent[o + r];
      if (c >= 0 && c < f.K) vote[c][lane] += s;
      if (fuse_view(f, sm, o, r)) m1 = fmaxf(m1, sc);
      else m0 = fmaxf(m0, sc);
    };
    if (lane == 0) member(p);
    const unsigned long long* row = mask + (long)p * nw;
    for (int w = (p >> 6) + lane; w < nw; w += 64) {
      unsigned long long bits = row[w];
      while (bits) {
        const long q = (long)w * 64 + __builtin_ctzll(bits);
        bits &= bits - 1ull;
        if (q < n && f.owner[o + q] == (int)j) member((int)q);
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) members += __shfl_xor(members, s, 64);
    float ob[5] = {bp[0], bp[1], bp[2], bp[3], bp[4]};
    float osc = f.score[o + rp];
    int oint = f.intent[o + rp];
    if (f.fuse) {
      S = wave_sum_f64(S);
      sx = wave_sum_f64(sx);
      sy = wave_sum_f64(sy);
      sw = wave_sum_f64(sw);
      sl = wave_sum_f64(sl);
      sd = wave_sum_f64(sd);
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        m0 = fmaxf(m0, __shfl_xor(m0, s, 64));
        m1 = fmaxf(m1, __shfl_xor(m1, s, 64));
      }
      double best = 0.0;
      int bc = 0;
      for (int c = 0; c < f.K; ++c) {
        const double v = wave_sum_f64(vote[c][lane]);
        if (c == 0 || v > best) {  // the lowest class wins a tie
          best = v;
          bc = c;
        }
      }
      oint = bc;
      if (S > 0.0) {  // a cluster without positive weight keeps the leader's box
        double a = ap + sd / S;
        if (a > FUSE_PI) a -= 2.0 * FUSE_PI;
        else if (a <= -FUSE_PI) a += 2.0 * FUSE_PI;
        ob[0] = (float)(sx / S);
        ob[1] = (float)(sy / S);
        ob[2] = (float)(sw / S);
        ob[3] = (float)(sl / S);
        ob[4] = (float)a;
      }
      const float z0 = m0 == -INFINITY ? 0.f : m0, z1 = m1 == -INFINITY ? 0.f : m1;
      osc = f.n_views == 2 ? (z0 + z1) * 0.5f : z0;
    }
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < 5; ++e) f.tbox[(o + j) * 5 + e] = ob[e];
      f.tscore[o + j] = osc;
      f.tint[o + j] = oint;
      f.tmem[o + j] = members;
    }
    __syncthreads();  // one wave: the next leader clears vote[] after every lane has read it
  }
}

// grid (samples). direct: no cluster stage ran (fuse = 0 and no member counts asked for); the rows
// are the leaders' own, read from the candidates.
__global__ __launch_bounds__(PS_T) void fuse_emit_kernel(FuseWs f, SegView sv, int direct, long* __restrict__ out_leader,
                                                         float* __restrict__ out_box, float* __restrict__ out_score,
                                                         long* __restrict__ out_int, int* __restrict__ out_mem) {
  __shared__ unsigned hist[PS_D * PS_T];
  __shared__ unsigned wsum[20];
  __shared__ int skip;
  const int sm = blockIdx.x;
  const long o = sv.lo(sm);
  const int cnt = (int)min(f.count[sm], sv.n(sm));
  const int* perm = nullptr;
  if (f.fuse && f.n_views == 2 && !direct) {
    for (int j = threadIdx.x; j < cnt; j += PS_T) {
      f.k0[o + j] = desc_key(f.tscore[o + j]);
      f.v0[o + j] = j;
    }
    __syncthreads();
    const int r = block_radix_sort(f.k0 + o, f.v0 + o, f.k1 + o, f.v1 + o, cnt, hist, wsum, &skip);
    perm = (r ? f.v1 : f.v0) + o;
  }
  for (int i = threadIdx.x; i < cnt; i += PS_T) {
    const int j = perm ? perm[i] : i;
    const long lr = f.keep[o + j];
    const float* b = direct ? f.box + (o + lr) * 5 : f.tbox + (o + j) * 5;
    if (out_leader) out_leader[o + i] = lr;
#pragma unroll
    for (int e = 0; e < 5; ++e) out_box[(o + i) * 5 + e] = b[e];
    out_score[o + i] = direct ? f.score[o + lr] : f.tscore[o + j];
    out_int[o + i] = direct ? f.intent[o + lr] : f.tint[o + j];
    if (out_mem) out_mem[o + i] = direct ? 1 : f.tmem[o + j];
  }
}

// The stages after the walk. keep / count: the walk's outputs.
void fuse_stages(const FuseWs& f, const SegView& sv, long samples, long max_n, long* out_leader, float* out_box,
                 float* out_score, long* out_int, int* out_mem, hipStream_t st) {
  const int direct = !f.fuse && !out_mem;
  if (!direct) {
    hipLaunchKernelGGL(fuse_rank_kernel, dim3(ivit_cdiv(max_n, 256), samples), dim3(256), 0, st, f, sv);
    hipLaunchKernelGGL(fuse_owner_kernel, dim3((int)min((long)64, (max_n + 3) / 4), samples), dim3(256), 0, st, f, sv);
    hipLaunchKernelGGL(fuse_cluster_kernel, dim3((int)min((long)256, max_n), samples), dim3(64), 0, st, f, sv);
  }
  hipLaunchKernelGGL(fuse_emit_kernel, dim3(samples), dim3(PS_T), 0, st, f, sv, direct, out_leader, out_box,
                     out_score, out_int, out_mem);
}

// The fusion scratch, placed behind the NMS workspace's regions: rank, owner, tscore, tint, tmem,
// each [rows] and rounded up to 16 bytes.
constexpr int FUSE_REGIONS = 5;
long fuse_extra_bytes(long rows) { return FUSE_REGIONS * al16(4 * rows); }
void fuse_extra(char* p, long rows, FuseWs& f) {
  const long step = al16(4 * rows);
  f.rank = (int*)p;
  f.owner = (int*)(p + step);
  f.tscore = (float*)(p + 2 * step);
  f.tint = (int*)(p + 3 * step);
  f.tmem = (int*)(p + 4 * step);
}

// ivit_nms_fuse_batched's workspace: BatchWs, then the walk's keep list (8 B per row), then the
// fusion scratch.
long fuse_batch_bytes(long n_samples, long total, long mask_words, bool rotated) {
  if (n_samples <= 0 || total <= 0) return 64;
  return batch_ws(nullptr, total, mask_words, rotated).bytes + al16(8 * total) + fuse_extra_bytes(total);
}

// ---- ivit_eval_post_tta: the selection of ivit_eval_post over V views of the same scenes ----------
struct TtaIn {
  const float* cls;     // [V, B, NA]
  const float* rel;     // [V, B, NA, 6]
  const float* intent;  // [V, B, NA, K]
  int B, NA, K, V;
  int flip[FUSE_MAXK];  // view 1: the intention a mirrored scene's class means in the original one
  int* cint;            // [B * V * NA] candidate intentions
  int* split;           // [B] rows of view 0
};

// torch's argmax over K logits: the first maximum; a NaN is the maximum, the first NaN wins
IVIT_DEV int argmax_first(const float* lg, int K) {
  int best = 0;
  float bv = lg[0];
  for (int e = 1; e < K; ++e) {
    const float v = lg[e];
    if (bv == bv && (v > bv || v != v)) {
      bv = v;
      best = e;
    }
  }
  return best;
}

// post_select_kernel for sample blockIdx.x with capacity V * NA rows: view 0's passing anchors in
// anchor order, then view 1's, un-mirrored (the inverse of the training flip: y and the yaw
// negated, both exactly; the intention through the table); every row's argmax intention; then the
// same stable descending sort and corner rows.
__global__ __launch_bounds__(PS_T) void post_select_tta_kernel(TtaIn in, const float* __restrict__ anchors, float conf,
                                                               PostWs w) {
  __shared__ unsigned hist[PS_D * PS_T];
  __shared__ unsigned wsum[20];
  __shared__ int skip;
  const int sm = blockIdx.x, t = threadIdx.x, NA = in.NA;
  const long base = (long)sm * in.V * NA;
  const int I = (NA + PS_T - 1) / PS_T;
  const int a0 = min(t * I, NA), a1 = min(a0 + I, NA);
  unsigned done = 0;
  for (int v = 0; v < in.V; ++v) {
    const long vb = ((long)v * in.B + sm) * NA;
    const float* c = in.cls + vb;
    const float* r = in.rel + vb * 6;
    unsigned np = 0;
    for (int g0 = a0; g0 < a1; g0 += 8) {
      float lr[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) lr[e] = g0 + e < a1 ? c[g0 + e] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) np += g0 + e < a1 && torch_sigmoid(lr[e]) >= conf;
    }
    unsigned p = done + block_excl_scan(np, wsum);
    const unsigned tot = wsum[16];
    for (int g0 = a0; g0 < a1; g0 += 8) {
      float lr[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) lr[e] = g0 + e < a1 ? c[g0 + e] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int a = g0 + e;
        const float s = torch_sigmoid(lr[e]);
        if (a < a1 && s >= conf) {
          const long q = base + p;
          w.anchor[q] = v * NA + a;
          w.score[q] = s;
          w.k0[q] = desc_key(s);
          w.v0[q] = (int)p;
          float o[5];
          decode_one(r + (long)a * 6, anchors + (long)a * 5, o);
          if (v) {
            o[1] = -o[1];
            o[4] = -o[4];
          }
#pragma unroll
          for (int k = 0; k < 5; ++k) w.box[q * 5 + k] = o[k];
          const int cl = argmax_first(in.intent + (vb + a) * in.K, in.K);
          in.cint[q] = v ? in.flip[cl] : cl;
          ++p;
        }
      }
    }
    if (t == 0 && v == 0) in.split[sm] = (int)tot;
    done += tot;
    __syncthreads();  // wsum[16] has been read by every thread before the next view's scan
  }
  const int n = (int)done;
  if (t == 0) w.n[sm] = n;
  __syncthreads();
  const int res = block_radix_sort(w.k0 + base, w.v0 + base, w.k1 + base, w.v1 + base, n, hist, wsum, &skip);
  const int* ord = (res ? w.v1 : w.v0) + base;
  for (int i = t; i < n; i += PS_T) {
    const int q = ord[i];
    w.order[base + i] = q;
    sorted_corners(w.box + (base + q) * 5, w.sb + (base + i) * 5);
  }
}

// ivit_eval_post_tta's workspace: ivit_eval_post's layout at capacity V * NA rows per sample, then
// the candidate intentions (4 B per row), the view-0 counts (4 B per sample), the fusion scratch.
long tta_ws_bytes(long B, long V, long NA, bool rotated) {
  if (B <= 0 || NA <= 0 || V <= 0) return 64;
  const long R = B * V * NA;
  return post_layout(B, V * NA, rotated).bytes + al16(4 * R) + al16(4 * B) + fuse_extra_bytes(R);
}
}  // namespace

extern "C" long ivit_nms_fuse_batched_workspace(long n_samples, long total, long mask_words, int rotated) {
  return fuse_batch_bytes(n_samples, total, mask_words, rotated != 0);
}

extern "C" int ivit_nms_fuse_batched(const float* boxes_xywha, const float* scores, const int* intentions,
                                     const int* views, const long* seg, const long* mask_off, long n_samples,
                                     long total, long max_n, long mask_words, long K, long n_views, int fuse,
                                     int rotated, double iou_thr, long* out_leader, float* out_boxes,
                                     float* out_scores, long* out_intent, int* out_members, long* count, void* work,
                                     long work_bytes, void* stream) {
  const char* name = "ivit_nms_fuse_batched";
  IVIT_CHECK_ARG(n_views == 1 || n_views == 2, "%s: n_views must be 1 or 2 (got %ld)", name, n_views);
  IVIT_CHECK_ARG(K >= 1 && K <= FUSE_MAXK, "%s: K must be in 1..%d (got %ld)", name, FUSE_MAXK, K);
  IVIT_CHECK_ARG(max_n <= 64L * NMS_MAXW, "%s: n=%ld exceeds %d", name, max_n, 64 * NMS_MAXW);
  IVIT_CHECK_ARG(n_samples >= 0 && n_samples < 65536 && total >= 0 && total < (1L << 31) && max_n >= 0 &&
                     mask_words >= 0,
                 "%s: bad sizes (samples %ld, rows %ld)", name, n_samples, total);
  IVIT_CHECK_ARG(work_bytes >= fuse_batch_bytes(n_samples, total, mask_words, rotated != 0), "%s: workspace too small",
                 name);
  IVIT_CHECK_ARG(intentions != nullptr || total == 0, "%s: intentions is null", name);
  hipStream_t st = ivit_stream(stream);
  if (n_samples <= 0) return 0;
  if (max_n <= 0 || total <= 0) {
    (void)hipMemsetAsync(count, 0, sizeof(long) * n_samples, st);
    return launch_status(name);
  }
  const BatchWs w = batch_ws(work, total, mask_words, rotated != 0);
  char* tail = (char*)(((uintptr_t)work + 15) & ~(uintptr_t)15) + (w.bytes - 64);
  long* keep = (long*)tail;
  const SegView sv{seg, mask_off, nullptr, 0, 0};
  hipLaunchKernelGGL(nms_sort_b_kernel, dim3(n_samples), dim3(PS_T), 0, st, boxes_xywha, scores, seg, w.k0, w.v0, w.k1,
                     w.v1, w.order, w.sb);
  nms_mask_and_scan(boxes_xywha, w.order, w.sb, w.rp, w.rc, w.mask, sv, n_samples, max_n, iou_thr, rotated != 0, keep,
                    count, st);
  FuseWs f{};
  f.box = boxes_xywha;
  f.score = scores;
  f.intent = intentions;
  f.views = n_views == 2 ? views : nullptr;
  f.order = w.order;
  f.keep = keep;
  f.count = count;
  f.mask = w.mask;
  f.tbox = w.sb;
  f.k0 = w.k0;
  f.k1 = w.k1;
  f.v0 = w.v0;
  f.v1 = w.v1;
  f.K = (int)K;
  f.n_views = (int)n_views;
  f.fuse = fuse != 0;
  fuse_extra(tail + al16(8 * total), total, f);
  fuse_stages(f, sv, n_samples, max_n, out_leader, out_boxes, out_scores, out_intent, out_members, st);
  return launch_status(name);
}

extern "C" long ivit_eval_post_tta_workspace(long B, long V, long NA, int rotated) {
  return tta_ws_bytes(B, V, NA, rotated != 0);
}

extern "C" int ivit_eval_post_tta(const float* cls, const float* box_rel, const float* intent, const float* anchors,
                                  long V, long B, long NA, long K, const int* flip_intent, float conf_thr,
                                  double iou_thr, int rotated, int fuse, float* out_scores, float* out_boxes,
                                  long* out_intent, int* out_members, long* out_count, void* work, long work_bytes,
                                  void* stream) {
  const char* name = "ivit_eval_post_tta";
  IVIT_CHECK_ARG(V == 1 || V == 2, "%s: V must be 1 or 2 (got %ld)", name, V);
  IVIT_CHECK_ARG(K >= 1 && K <= FUSE_MAXK, "%s: K must be in 1..%d (got %ld)", name, FUSE_MAXK, K);
  IVIT_CHECK_ARG(B >= 0 && B < 65536 && NA >= 0, "%s: bad sizes (B %ld, NA %ld)", name, B, NA);
  IVIT_CHECK_ARG(V * NA <= 64L * NMS_MAXW, "%s: V*NA=%ld exceeds %d", name, V * NA, 64 * NMS_MAXW);
  IVIT_CHECK_ARG(B * V * NA < (1L << 31), "%s: too many rows (%ld)", name, B * V * NA);
  TtaIn in{};
  for (int k = 0; k < (int)K; ++k) {
    in.flip[k] = flip_intent ? flip_intent[k] : k;
    IVIT_CHECK_ARG(in.flip[k] >= 0 && in.flip[k] < K, "%s: flip_intent[%d]=%d outside 0..%ld", name, k, in.flip[k],
                   K - 1);
  }
  IVIT_CHECK_ARG(work_bytes >= tta_ws_bytes(B, V, NA, rotated != 0), "%s: workspace too small", name);
  hipStream_t st = ivit_stream(stream);
  if (B == 0) return 0;
  if (NA == 0) {
    (void)hipMemsetAsync(out_count, 0, sizeof(long) * B, st);
    return launch_status(name);
  }
  const long C = V * NA, R = B * C;
  const PostWs w = post_ws(work, B, C, rotated != 0);
  char* tail = (char*)(((uintptr_t)work + 15) & ~(uintptr_t)15) + (post_layout(B, C, rotated != 0).bytes - 16);
  in.cls = cls;
  in.rel = box_rel;
  in.intent = intent;
  in.B = (int)B;
  in.NA = (int)NA;
  in.K = (int)K;
  in.V = (int)V;
  in.cint = (int*)tail;
  in.split = (int*)(tail + al16(4 * R));
  const SegView sv{nullptr, nullptr, w.n, C, C * ((C + 63) / 64)};
  hipLaunchKernelGGL(post_select_tta_kernel, dim3(B), dim3(PS_T), 0, st, in, anchors, conf_thr, w);
  nms_mask_and_scan(w.box, w.order, w.sb, w.rp, w.rc, w.mask, sv, B, C, iou_thr, rotated != 0, w.keep, out_count, st);
  FuseWs f{};
  f.box = w.box;
  f.score = w.score;
  f.intent = in.cint;
  f.split = V == 2 ? in.split : nullptr;
  f.order = w.order;
  f.keep = w.keep;
  f.count = out_count;
  f.mask = w.mask;
  f.tbox = w.sb;
  f.k0 = w.k0;
  f.k1 = w.k1;
  f.v0 = w.v0;
  f.v1 = w.v1;
  f.K = (int)K;
  f.n_views = (int)V;
  f.fuse = fuse != 0;
  fuse_extra(tail + al16(4 * R) + al16(4 * B), R, f);
  fuse_stages(f, sv, B, C, nullptr, out_boxes, out_scores, out_intent, out_members, st);
  return launch_status(name);
}
