// Flash attention forward + backward for gfx950 (K1/K2 in SURVEY.md §2.11): the round-1/2
// kernels, now the FALLBACKS -- the forward for offsets past 2 GB (attn_fwd.hip addresses 32-bit
// buffer offsets), the fused backward (fp32-atomic dQ) for shapes attn_bwd_split.hip cannot
// address, and the A/B form of the split backward (attn_bwd flags 8).  Round 4 removed the
// 256-key fused backward (v2) that no default path selected.
//
// bf16 in/out, fp32 accumulation, online softmax in base 2, causal or full,
// GQA (Hq a multiple of Hkv), head dim D in {64, 128}.  Q/K/V/O are addressed
// through (batch, token, head) element strides, so the packed (B, T, 3, H, D)
// output of a fused QKV projection is consumed in place and O is written as
// (B, T, H, D) -- no transposes around the kernel.
//
// MFMA: v_mfma_f32_32x32x16_bf16 everywhere (A 32x16, B 16x32, C 32x32 with
// C[row=(r&3)+8(r>>2)+4(l>>5)][col=l&31]).
//
// Forward (one 256-thread workgroup = 4 waves = 128 query rows, KV tiles of
// 64 keys, double-buffered in LDS, one barrier per tile):
//   * S^T = K Q^T ("swapped"): the query index is the MFMA column = the lane,
//     so a lane holds 32 scores of ONE query; the row max / row sum need a
//     single cross-half exchange (lane ^ 32) instead of a 32-lane butterfly;
//   * the S^T accumulator, rounded to bf16, IS the B operand of
//     O^T += V^T P^T (k order permuted inside a 16-key step; V^T is gathered
//     with the matching permutation by ds_read_b64_tr_b16, the gfx950
//     transposing LDS read), so P never touches LDS;
//   * O^T also has the query on the lane: the online-softmax rescale is one
//     per-lane scalar multiply.
// Backward (one workgroup = 4 waves = 128 keys, 32 keys per wave, loop over
// query tiles of 32 rows and over the Hq/Hkv query heads of the KV head):
//   * S = Q K^T and dP = dO V^T with the KEY on the lane; K and V fragments
//     stay in registers for the whole kernel;
//   * dV^T += dO^T P and dK^T += Q^T dS take the S/dP accumulators directly as
//     B operands (no LDS), accumulating in registers across all query tiles;
//   * only dS crosses LDS (one 2 KB transposed image per wave) for
//     dQ = dS K; the 4 waves' dQ partials are folded in LDS and added to an
//     fp32 dQ buffer with one 256-byte float-atomic row per wave instruction.
//
// LDS images: 16-byte chunk c of row r lives at chunk c ^ f(r) with
//   D=128: f = ((r&3)<<2)|((r>>2)&3)          (256-B rows)
//   D=64 : f = ((r>>1)&1)<<2 | ((r>>3)&1)<<1 | ((r>>2)&1)   (128-B rows)
// which makes BOTH the row reads (ds_read_b128, 16 distinct rows per lane
// group) and the transposed reads (4 rows x 32 columns per half-wave)
// conflict-free on the 64-bank LDS.
#include <type_traits>

#include "common.h"
#include "launchers.h"
#include "lds_once.h"
#include "mfma_lds.h"

namespace orion {



// ============================================================================ forward
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnParams p) {
  constexpr int BM = 128, BN = 64, NCH = D / 8, TILE = BN * D, NST = BN * NCH / 256;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];  // [2 bufs][K|V][TILE]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h32 = lane >> 5, l32 = lane & 31;
  const int BH = p.B * p.Hq;
  const int nqt = (p.T + BM - 1) / BM;
  const int bh = blockIdx.x % BH;
  const int qt = nqt - 1 - (int)(blockIdx.x / BH);  // heaviest (causal) tiles launch first
  const int b = bh / p.Hq, hq = bh % p.Hq, hk = hq / (p.Hq / p.Hkv);
  const int q0 = qt * BM, qw0 = q0 + wv * 32;
  const int off = p.Tk - p.T;  // causal: key <= query + off
  const float c = p.scale_log2;

  const bf16_t* Qb = p.q + b * p.q_sb + hq * p.q_sh;
  const bf16_t* Kb = p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* Vb = p.v + b * p.v_sb + hk * p.v_sh;

  bf16x8 qf[D / 16];
  {
    const int qr = min(qw0 + l32, p.T - 1);
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks)
      qf[ks] = *reinterpret_cast<const bf16x8*>(Qb + (long)qr * p.q_st + ks * 16 + 8 * h32);
  }
  const int kend = CAUSAL ? min(p.Tk, q0 + BM + off) : p.Tk;
  const int ntiles = (kend + BN - 1) / BN;

  bf16x8 kst[NST], vst[NST];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int cidx = tid + i * 256, row = cidx / NCH, ch = cidx % NCH;
      const long key = min(t * BN + row, p.Tk - 1);
      kst[i] = *reinterpret_cast<const bf16x8*>(Kb + key * p.k_st + ch * 8);
      vst[i] = *reinterpret_cast<const bf16x8*>(Vb + key * p.v_st + ch * 8);
    }
  };
  auto swrite = [&](int buf) {
    bf16_t* Ks = smem + buf * 2 * TILE;
    bf16_t* Vs = Ks + TILE;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int cidx = tid + i * 256, row = cidx / NCH, ch = cidx % NCH;
      const int o = loff<D>(row, ch * 8);
      *reinterpret_cast<bf16x8*>(Ks + o) = kst[i];
      *reinterpret_cast<bf16x8*>(Vs + o) = vst[i];
    }
  };

  f32x16 oacc[D / 32];
#pragma unroll
  for (int db = 0; db < D / 32; ++db) oacc[db] = zero16();
  float m = -1e30f, lsum = 0.f;
  const int myq = qw0 + l32;

  // Staging (issue early, write late): tile t+1 sits in registers while tile t is computed;
  // right after the barrier that ends tile t-1 it is written to the LDS buffer tile t-1 used,
  // and tile t+2's loads are issued -- so the LDS writes overlap this tile's MFMAs instead
  // of delaying the barrier, and each load has a whole tile of compute to land.
  gload(0);
  swrite(0);
  // Retire EVERY prologue load (Q fragments included) with an s_waitcnt the compiler's
  // wait-count pass can see.  Without it the pass treats qf as still in flight at the loop
  // header and makes the first QK^T MFMAs of every tile wait vmcnt(3..0) -- i.e. on the
  // NEXT tile's prefetch -- exposing a full HBM round trip per tile.
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  if (ntiles > 1) gload(1);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) swrite((t + 1) & 1);
    if (t + 2 < ntiles) gload(t + 2);
    const int k0 = t * BN;
    const bf16_t* Ks = smem + (t & 1) * 2 * TILE;
    const bf16_t* Vs = Ks + TILE;
    const bool active = !CAUSAL || (k0 <= qw0 + 31 + off);
    if (active) {
      f32x16 s[2];
      bf16x8 kfr[2][D / 16];  // all K fragments of the tile: reads issue back to back
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks)
          kfr[kb][ks] = lds_b128(Ks, loff<D>(kb * 32 + l32, ks * 16 + 8 * h32));
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        s[kb] = zero16();
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) s[kb] = mfma32(kfr[kb][ks], qf[ks], s[kb]);
      }
      const bool need_mask = (CAUSAL && (k0 + BN - 1 > qw0 + off)) || (k0 + BN > p.Tk);
      if (need_mask) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h32;
            if (key >= p.Tk || (CAUSAL && key > myq + off)) s[kb][r] = -INFINITY;
          }
      }
      float mx = m;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // deferred rescale: keep the running max while no row of the wave grew by more than
      // 8 (log2 units), so P stays <= 2^8 (exact in fp32 sums, bf16-rounded like any P); the
      // O / l rescale pass then runs only on the tiles that raise a row's max that much
      float alpha = 1.f;
      if (__any((mx - m) * c > 8.f)) {
        alpha = __builtin_amdgcn_exp2f((m - mx) * c);
        m = mx;
#pragma unroll
        for (int db = 0; db < D / 32; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
      }
      const float mc = m * c;
      float ps = 0.f;
      bf16x8 pf[4];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[kb][8 * s2 + j], c, -mc));
            ps += e;
            pf[kb * 2 + s2][j] = f2bf(e);
          }
      lsum = lsum * alpha + ps;
#pragma unroll
      for (int db = 0; db < D / 32; ++db) {
        bf16x8 vfr[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) vfr[kk] = tr_frag<D>(Vs, kk * 16 + 4 * h32, db * 32, lane, 8);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) oacc[db] = mfma32(vfr[kk], pf[kk], oacc[db]);
      }
    }
    __syncthreads();
  }

  const float lt = lsum + __shfl_xor(lsum, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (myq < p.T) {
    bf16_t* Ob = p.o + b * p.o_sb + hq * p.o_sh + (long)myq * p.o_st;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = f2bf(oacc[db][4 * g4 + j] * inv);
        *reinterpret_cast<bf16x4*>(Ob + db * 32 + 8 * g4 + 4 * h32) = v4;
      }
    if (h32 == 0) p.lse[((long)b * p.Hq + hq) * p.T + myq] = m * c + __log2f(lt);
  }
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also emits
// s_waitcnt vmcnt(0), which in the backward made every query-tile iteration wait for
// its own dQ atomics to complete (a full atomic round trip per iteration); the atomics
// have no reader inside the kernel, so they may stay in flight across the barrier.
// The "memory" clobber keeps the compiler from moving LDS accesses across it.
ORION_DEVICE void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ============================================================================ backward prep
// delta[b][h][t] = sum_d dO * O ; 8 bf16 per lane, D/8 lanes per row.  Also zeroes the
// row's fp32 dQ accumulator (the backward adds into it with atomics): a kernel, not a
// hipMemsetAsync -- inside a captured HIP graph the memset node raced the atomics
// (wrong / NaN gradients on replay that came and went with timing).
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_pre_kernel(AttnParams p, float* delta) {
  constexpr int TPR = D / 8;  // threads per row
  const long row = (blockIdx.x * 256L + threadIdx.x) / TPR;
  const int sub = threadIdx.x % TPR;
  const long nrows = (long)p.B * p.Hq * p.T;
  float s = 0.f;
  long b = 0, h = 0, t = 0;
  if (row < nrows) {
    t = row % p.T;
    h = (row / p.T) % p.Hq;
    b = row / ((long)p.T * p.Hq);
    const bf16x8 o = *reinterpret_cast<const bf16x8*>(p.o + b * p.o_sb + h * p.o_sh + t * p.o_st + sub * 8);
    const bf16x8 d = *reinterpret_cast<const bf16x8*>(p.dout + b * p.do_sb + h * p.do_sh + t * p.do_st + sub * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bf2f(o[j]) * bf2f(d[j]);
  }
#pragma unroll
  for (int o2 = TPR / 2; o2 > 0; o2 >>= 1) s += __shfl_xor(s, o2, 64);
  if (row < nrows) {
    if (sub == 0) delta[row] = s;
    f32x4* z = reinterpret_cast<f32x4*>(p.dq_acc + row * D + sub * 8);
    z[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    z[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ============================================================================ backward
template <int D, bool CAUSAL>
__global__ __launch_bounds__(bwd_waves<D>() * 64, (D == 64 ? 2 : 1)) void attn_bwd_kernel(AttnParams p) {
  constexpr int NW = bwd_waves<D>(), NT = NW * 64;
  constexpr int BNK = 32 * NW, BMQ = 32, NCH = D / 8;
  constexpr int KT = BNK * D;  // K image elements
  constexpr int QT = BMQ * D;  // Q / dO tile elements
  constexpr int NQC = BMQ * NCH;          // 16-byte chunks per Q (or dO) tile
  constexpr int NSTQ = 2 * NQC / NT;      // chunks per thread per Q+dO stage
  static_assert(NSTQ * NT == 2 * NQC, "Q/dO staging must divide over the threads");
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  bf16_t* Ks = smem;                       // [BNK][D]
  bf16_t* Qs = Ks + KT;                    // [2][32][D]
  bf16_t* Ds = Qs + 2 * QT;                // [2][32][D]  (dO)
  bf16_t* St = Ds + 2 * QT;                // [NW waves][32 keys][32 q]
  float* lse_s = reinterpret_cast<float*>(St + NW * 32 * 32);  // [2][32]
  float* del_s = lse_s + 64;                                   // [2][32]
  constexpr int DQP = BMQ + 4;  // padded q-row of the [d][q] dQ partials (conflict-free b128)
  float* dqr = del_s + 64;                                     // [NW][D][DQP]

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h32 = lane >> 5, l32 = lane & 31;
  const int BHk = p.B * p.Hkv;
  const int kt = blockIdx.x / BHk;  // small kt = most work under the causal mask: first
  const int bh = blockIdx.x % BHk;
  const int b = bh / p.Hkv, hk = bh % p.Hkv;
  const int rep = p.Hq / p.Hkv;
  const int kt0 = kt * BNK, kw0 = kt0 + wv * 32;
  const int off = p.Tk - p.T;
  const float c = p.scale_log2;

  const bf16_t* Kb = p.k + b * p.k_sb + hk * p.k_sh;
  const bf16_t* Vb = p.v + b * p.v_sb + hk * p.v_sh;

  // K/V fragments of this wave's 32 keys (B operands of S and dP), kept in registers
  bf16x8 kf[D / 16], vf[D / 16];
  {
    const long key = min(kw0 + l32, p.Tk - 1);
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(Kb + key * p.k_st + ks * 16 + 8 * h32);
      vf[ks] = *reinterpret_cast<const bf16x8*>(Vb + key * p.v_st + ks * 16 + 8 * h32);
    }
  }
  // K image for the dQ product (transposed reads)
  for (int cidx = tid; cidx < BNK * NCH; cidx += NT) {
    const int row = cidx / NCH, ch = cidx % NCH;
    const long key = min(kt0 + row, p.Tk - 1);
    *reinterpret_cast<bf16x8*>(Ks + loff<D>(row, ch * 8)) =
        *reinterpret_cast<const bf16x8*>(Kb + key * p.k_st + ch * 8);
  }

  f32x16 dka[D / 32], dva[D / 32];
#pragma unroll
  for (int db = 0; db < D / 32; ++db) { dka[db] = zero16(); dva[db] = zero16(); }

  // first query row that can see any key of this workgroup
  const int qlo = CAUSAL ? max(0, kt0 - off) : 0;
  const int qi0 = qlo / BMQ;
  const int nqi = (p.T + BMQ - 1) / BMQ;
  const int iters_per_head = nqi - qi0;
  const int total = iters_per_head * rep;

  // Q+dO staging registers (NSTQ 16-byte chunks per thread)
  bf16x8 qdst[NSTQ];
  float lse_r = 0.f, del_r = 0.f;
  auto gload = [&](int it) {
    const int hq = hk * rep + it / iters_per_head;
    const int qbase = (qi0 + it % iters_per_head) * BMQ;
    const bf16_t* Qb = p.q + b * p.q_sb + hq * p.q_sh;
    const bf16_t* Db = p.dout + b * p.do_sb + hq * p.do_sh;
    if constexpr (NSTQ >= 2) {  // each thread: NSTQ/2 chunks of Q and the same of dO
#pragma unroll
      for (int i = 0; i < NSTQ / 2; ++i) {
        const int c = tid + i * NT, row = c / NCH, ch = c % NCH;
        const long q = min(qbase + row, p.T - 1);
        qdst[i] = *reinterpret_cast<const bf16x8*>(Qb + q * p.q_st + ch * 8);
        qdst[NSTQ / 2 + i] = *reinterpret_cast<const bf16x8*>(Db + q * p.do_st + ch * 8);
      }
    } else {  // one chunk per thread: the first NQC threads take Q, the rest dO
      const int isd = tid >= NQC, w = tid - isd * NQC;
      const long q = min(qbase + w / NCH, p.T - 1);
      const bf16_t* src = isd ? Db + q * p.do_st : Qb + q * p.q_st;
      qdst[0] = *reinterpret_cast<const bf16x8*>(src + (w % NCH) * 8);
    }
    if (tid < 32) {
      const long q = min(qbase + tid, p.T - 1);
      const long r = ((long)b * p.Hq + hq) * p.T + q;
      lse_r = p.lse[r];
      del_r = p.delta[r];
    }
  };
  auto swrite = [&](int buf) {
    if constexpr (NSTQ >= 2) {
#pragma unroll
      for (int i = 0; i < NSTQ / 2; ++i) {
        const int c = tid + i * NT, o = loff<D>(c / NCH, (c % NCH) * 8);
        *reinterpret_cast<bf16x8*>(Qs + buf * QT + o) = qdst[i];
        *reinterpret_cast<bf16x8*>(Ds + buf * QT + o) = qdst[NSTQ / 2 + i];
      }
    } else {
      const int isd = tid >= NQC, w = tid - isd * NQC;
      *reinterpret_cast<bf16x8*>((isd ? Ds : Qs) + buf * QT + loff<D>(w / NCH, (w % NCH) * 8)) = qdst[0];
    }
    if (tid < 32) {
      lse_s[buf * 32 + tid] = lse_r;
      del_s[buf * 32 + tid] = del_r;
    }
  };

  bf16_t* Sw = St + wv * 32 * 32;
  float* dqw = dqr + wv * D * DQP;
  const int mykey = kw0 + l32;

  if (total > 0) {
    gload(0);
    swrite(0);
  }
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int buf = it & 1;
    const int hq = hk * rep + it / iters_per_head;
    const int qbase = (qi0 + it % iters_per_head) * BMQ;
    if (it + 1 < total) gload(it + 1);
    const bf16_t* Qc = Qs + buf * QT;
    const bf16_t* Dc = Ds + buf * QT;
    const bool active = !CAUSAL || (qbase + BMQ - 1 + off >= kw0);
    f32x16 dq[D / 32];
    if (active) {
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const int o = loff<D>(l32, ks * 16 + 8 * h32);
        s = mfma32(lds_b128(Qc, o), kf[ks], s);
        dp = mfma32(lds_b128(Dc, o), vf[ks], dp);
      }
      // P and dS in place (row q = (r&3)+8(r>>2)+4*h32 of this tile, column = mykey)
      const bool need_mask = (CAUSAL && (qbase + off < kw0 + 31)) || (kw0 + 32 > p.Tk) ||
                             (qbase + BMQ > p.T);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 L = *reinterpret_cast<const f32x4*>(lse_s + buf * 32 + 8 * g4 + 4 * h32);
        const f32x4 Dl = *reinterpret_cast<const f32x4*>(del_s + buf * 32 + 8 * g4 + 4 * h32);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g4 + j;
          float pv = __builtin_amdgcn_exp2f(fmaf(s[r], c, -L[j]));
          if (need_mask) {
            const int q = qbase + 8 * g4 + 4 * h32 + j;
            if (mykey >= p.Tk || q >= p.T || (CAUSAL && mykey > q + off)) pv = 0.f;
          }
          s[r] = pv;
          dp[r] = pv * (dp[r] - Dl[j]);  // dS / scale: the scale is applied to dK and dQ once
        }
      }
      bf16x8 pb[2], sb[2];
      pb[0] = acc_to_frag(s, 0);
      pb[1] = acc_to_frag(s, 1);
      sb[0] = acc_to_frag(dp, 0);
      sb[1] = acc_to_frag(dp, 1);
#pragma unroll
      for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          dva[db] = mfma32(tr_frag<D>(Dc, 16 * s2 + 4 * h32, db * 32, lane, 8), pb[s2], dva[db]);
          dka[db] = mfma32(tr_frag<D>(Qc, 16 * s2 + 4 * h32, db * 32, lane, 8), sb[s2], dka[db]);
        }
      // dS^T image [key][q]: 64-byte rows of eight 8-byte chunks (4 q each), chunk c of
      // row k stored at c ^ ((k>>1)&7).  The ds_write_b64 of 16 consecutive keys was 8-way
      // bank-conflicted unswizzled (PMC: 31% of LDS cycles were conflicts); the transposed
      // read (4 whole rows per half-wave) is conflict-free either way.
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = sb[g4 >> 1][4 * (g4 & 1) + j];
        *reinterpret_cast<bf16x4*>(Sw + l32 * 32 + 4 * ((2 * g4 + h32) ^ ((l32 >> 1) & 7))) = v4;
      }
      // dQ partial = dS K over this wave's 32 keys (A and B both by transposed reads)
      {
        const int g = lane >> 4, i = lane & 15;
#pragma unroll
        for (int db = 0; db < D / 32; ++db) dq[db] = zero16();
#pragma unroll
        for (int s3 = 0; s3 < 2; ++s3) {
          const int krow = 16 * s3 + 8 * h32 + (i >> 2);
          const int qcol = 16 * (g & 1) + 4 * (i & 3);
          const bf16x8 a = cat8(lds_tr(Sw, krow * 32 + 4 * ((qcol >> 2) ^ ((krow >> 1) & 7))),
                                lds_tr(Sw, (krow + 4) * 32 + 4 * ((qcol >> 2) ^ (((krow + 4) >> 1) & 7))));
#pragma unroll
          for (int db = 0; db < D / 32; ++db) {
            const bf16x8 bk = tr_frag<D>(Ks, wv * 32 + 16 * s3 + 8 * h32, db * 32, lane, 4);
            dq[db] = mfma32(a, bk, dq[db]);
          }
        }
      }
    } else {
#pragma unroll
      for (int db = 0; db < D / 32; ++db) dq[db] = zero16();
    }
    // per-wave dQ partial -> LDS as [d][q] (rows of DQP floats): accumulator registers
    // 4g..4g+3 are 4 consecutive q of one d, so each goes out as ONE 16-byte write
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = dq[db][4 * g4 + j];
        *reinterpret_cast<f32x4*>(dqw + (db * 32 + l32) * DQP + 8 * g4 + 4 * h32) = v;
      }
    if (it + 1 < total) swrite(buf ^ 1);
    lds_barrier();
    // fold the NW waves (16-byte reads of 4 q's) and add scale * sum to the fp32 dQ
    // accumulator: lanes run over d, so each atomic instruction covers D contiguous floats
    {
      float* dqg = p.dq_acc + (((long)b * p.Hq + hq) * p.T) * D;
      static_assert((BMQ * D / 4) % NT == 0, "fold groups must divide over the threads");
#pragma unroll
      for (int k = 0; k < BMQ * D / 4 / NT; ++k) {
        const int e = tid + k * NT;
        const int d = e % D, qg = e / D;
        const int o = d * DQP + 4 * qg;
        f32x4 sum = *reinterpret_cast<const f32x4*>(dqr + o);
#pragma unroll
        for (int w = 1; w < NW; ++w) sum += *reinterpret_cast<const f32x4*>(dqr + w * D * DQP + o);
        if (!(p.flags & 1)) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = qbase + 4 * qg + j;
            if (q < p.T) atomicAdd(dqg + (long)q * D + d, sum[j] * p.scale);
          }
        }
      }
    }
    lds_barrier();
  }

  // dK / dV: lane = key, registers = d ((r&3)+8(r>>2)+4*h32)
  if (mykey < p.Tk) {
    bf16_t* dKb = p.dk + b * p.dk_sb + hk * p.dk_sh + (long)mykey * p.dk_st;
    bf16_t* dVb = p.dv + b * p.dv_sb + hk * p.dv_sh + (long)mykey * p.dv_st;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 k4, v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          k4[j] = f2bf(dka[db][4 * g4 + j] * p.scale);
          v4[j] = f2bf(dva[db][4 * g4 + j]);
        }
        *reinterpret_cast<bf16x4*>(dKb + db * 32 + 8 * g4 + 4 * h32) = k4;
        *reinterpret_cast<bf16x4*>(dVb + db * 32 + 8 * g4 + 4 * h32) = v4;
      }
  }
}

template <int D>
__global__ __launch_bounds__(256) void attn_dq_convert_kernel(const float* __restrict__ acc,
                                                              bf16_t* __restrict__ dq, long sb,
                                                              long st, long sh, int B, int Hq,
                                                              int T) {
  const long n8 = (long)B * Hq * T * (D / 8);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long e = i * 8;
    const int d = e % D;
    const long row = e / D;
    const long t = row % T, h = (row / T) % Hq, b = row / ((long)T * Hq);
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(acc + e);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(acc + e + 4);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = f2bf(a0[j]); o[4 + j] = f2bf(a1[j]); }
    *reinterpret_cast<bf16x8*>(dq + b * sb + h * sh + t * st + d) = o;
  }
}

}  // namespace orion

using namespace orion;

extern "C++" {

// the 64-bit-addressed forward: past 2 GB of K / V, or ORION_ATTN_FWD=v2 (csrc/attn_plan.h)
int orion_attn_fwd64(const AttnLaunch& l, const AttnParams& p, int D, bool causal, hipStream_t st) {
  return attn_dispatch(D, causal, [&](auto d, auto c) {
    return launch_dynamic_lds<attn_fwd_kernel<d(), c()>>(l.grid, l.block, l.lds, st, p);
  });
}

int orion_attn_bwd(const AttnBwdPlan& plan, const AttnParams& p, int D, bool causal, float* delta,
                   hipStream_t st) {
  if (plan.form != ATTN_FUSED) return -1;  // step 0: attn_bwd_pre, step 1: attn_bwd
  AttnParams q = p;
  q.delta = delta;
  const AttnLaunch &pre = plan.step[0], &bwd = plan.step[1];
  return attn_dispatch(D, causal, [&](auto d, auto c) {
    attn_bwd_pre_kernel<d()><<<pre.grid, pre.block, pre.lds, st>>>(q, delta);
    return launch_dynamic_lds<attn_bwd_kernel<d(), c()>>(bwd.grid, bwd.block, bwd.lds, st, q);
  });
}

int orion_attn_dq_convert(const float* acc, void* dq, long sb, long st_, long sh, int B, int Hq,
                          int T, int D, hipStream_t st) {
  const long n8 = (long)B * Hq * T * (D / 8);
  long g = (n8 + 255) / 256;
  if (g > 4096) g = 4096;
  if (D == 64)
    attn_dq_convert_kernel<64><<<(int)g, 256, 0, st>>>(acc, (bf16_t*)dq, sb, st_, sh, B, Hq, T);
  else if (D == 128)
    attn_dq_convert_kernel<128><<<(int)g, 256, 0, st>>>(acc, (bf16_t*)dq, sb, st_, sh, B, Hq, T);
  else
    return -1;
  return (int)hipGetLastError();
}

}  // extern "C++"
