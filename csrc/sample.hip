// Token sampling on the device for the decode step on gfx950 (wave64, bf16 logits, fp32 math):
//   token[b] ~ softmax(logits[b] / T) over the entries >= the top_k-th largest of the row.
//
// sample_kernel<STAGED>, grid B, 1024 threads: one workgroup per row.
//   * Keys.  A bf16 logit becomes a 16-bit key whose unsigned order is the order of the floats
//     (sign bit flipped for positives, all bits for negatives; -0 takes +0's key, which frees
//     0x7fff as the mark of "no element").  The temperature is positive, so the order of
//     z = logit / T is the order of the keys and the top-k threshold is found on the keys alone.
//   * Layout.  The row is cut into 16-byte slots of 8 keys in *aligned* coordinates (element i
//     sits at a + i, a = the row's misalignment in elements, so a 2-byte aligned row of an odd V
//     still moves as aligned 16-byte vectors; the two edge slots are loaded element by element
//     and nothing outside [0, V) is read).  Thread t owns the `cs` contiguous slots from t cs, cs
//     odd: with the row staged in LDS (coalesced loads, slot j by thread j mod 1024) a wave's
//     ds_read_b128 at a stride of cs 16-byte units is bank-conflict free.  Rows of more than
//     SP_STAGE_SLOTS slots (Llama-3's 128,256) are not staged: each pass re-reads the thread's
//     range from the L2 with the same 16-byte loads.
//   * Threshold: exact two-pass radix select, a 256-bin histogram of the high byte then of the
//     low byte among the keys of the chosen high byte.  The bins are integer LDS atomics, 16
//     copies by lane (bf16's high byte is sign + 7 exponent bits: a few bins take every add);
//     a suffix scan by one wave picks the digit.  Entries with key >= threshold are kept, ties
//     included.  top_k <= 0 or >= V skips the select.
//   * Draw: w = exp(z - max z) over the kept entries; each thread sums its range in index
//     order, a fixed-order scan (shuffles in a wave, wave totals in wave order) gives each
//     thread the sum before its range and Z.  The first thread whose running sum exceeds u Z
//     walks its range again (the same additions) and stores the first index that exceeds it;
//     only a thread with weight of its own can be that thread, and only an entry of positive
//     weight that index.  If rounding leaves none, the last kept index of positive weight is
//     stored (the last kept index when there is none: NaN or -inf rows).  No float atomics: two launches on
//     the same inputs store the same tokens.
//   * u is given, or Philox4x32-10 with the 64-bit seed as key and (positions[b], b, 0, 0) as
//     counter: no state is advanced, so workgroups do not race.  With R > 1 rows per sequence (a
//     verify step of speculative decoding) row r is token r % R of sequence s = r / R and draws
//     from (positions[s] + pos_off + r % R, s, 0, 0): the counter a one-row step at that position
//     would use.
//   * A row of NaN or of -inf only makes every comparison false and takes the last-kept exit, so
//     the token stays in [0, V).
#include <limits.h>

#include "common.h"
#include "launchers.h"
#include "lds_once.h"

namespace orion {

namespace {

constexpr int SP_NT = 1024, SP_NW = SP_NT / 64;
constexpr int SP_COPIES = 16;                // histogram copies, by lane & 15
constexpr unsigned SP_NONE = 0x7fffu;        // key of no element
constexpr int SP_STAGE_SLOTS = 8192;         // 128 KiB of the 160 KiB LDS

ORION_DEVICE unsigned sp_key(unsigned b) {  // bf16 bits -> order-preserving key
  const unsigned k = (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
  return k == SP_NONE ? 0x8000u : k;  // -0 -> +0
}

ORION_DEVICE float sp_value(unsigned k) {  // key -> the logit
  const unsigned b = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}

// Slot j of the row as 8 keys, two per word (element e in half e & 1 of word e >> 1); elements
// outside [0, V) are SP_NONE.
ORION_DEVICE u32x4 sp_load_slot(const bf16_t* row, int a, int V, int j) {
  const long i0 = 8L * j - a;  // row index of the slot's first element
  unsigned k[8];
  if (i0 >= 0 && i0 + 8 <= V) {
    ORION_DASSERT((reinterpret_cast<uintptr_t>(row + i0) & 15) == 0);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(row + i0);
#pragma unroll
    for (int e = 0; e < 8; ++e) k[e] = sp_key(v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long i = i0 + e;
      k[e] = SP_NONE;
      if (i >= 0 && i < V) k[e] = sp_key(row[i]);
    }
  }
  return u32x4{k[0] | (k[1] << 16), k[2] | (k[3] << 16), k[4] | (k[5] << 16), k[6] | (k[7] << 16)};
}

ORION_DEVICE unsigned sp_elem(const u32x4& s, int e) { return (s[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }

ORION_DEVICE unsigned sp_philox_x0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// The digit d with count(bins > d) < k <= count(bins >= d) of the 256 bins in `bins`, by wave 0;
// out[0] = d, out[1] = k - count(bins > d).  Exactly one lane finds it when 1 <= k <= total.
ORION_DEVICE void sp_pick_digit(const int* bins, int k, int lane, int* out) {
  int c[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c[i] = bins[4 * lane + i];
    s += c[i];
  }
  int suf = s;  // bins of this lane and of every higher one
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += v;
  }
  int above = suf - s;
  if (above < k && k <= suf) {
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if (above < k && k <= above + c[i]) {
        out[0] = 4 * lane + i;
        out[1] = k - above;
      }
      above += c[i];
    }
  }
}

}  // namespace

template <bool STAGED>
__global__ __launch_bounds__(SP_NT) void sample_kernel(const SampleParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_dyn[];
  u32x4* sm = reinterpret_cast<u32x4*>(sp_dyn);  // STAGED: the row's slots
  __shared__ int hist[256 * SP_COPIES];
  __shared__ int bins[256];
  __shared__ float wtot[SP_NW];
  __shared__ int pick[2];
  __shared__ int s_max, s_first, s_last, s_lastw;
  __shared__ float s_u;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x, V = p.V;
  ORION_DASSERT(b < p.B && V >= 1);
  const bf16_t* row = p.logits + (long)b * p.logits_rs;
  const int a = (int)((reinterpret_cast<uintptr_t>(row) & 15) >> 1);
  const int nslots = (int)(((long)a + V + 7) >> 3);
  const int cs = ((nslots + SP_NT - 1) / SP_NT) | 1;  // slots per thread, odd
  const long jt = (long)tid * cs;
  const int j0 = (int)(jt < nslots ? jt : nslots), j1 = (int)(jt + cs < nslots ? jt + cs : nslots);

  const float t = fmaxf(__int_as_float(p.params[0]), 1e-6f);
  const int top_k = p.params[1];
  const bool select = top_k > 0 && top_k < V;

  if (tid == 0) {
    float u;
    if (p.u) {
      u = p.u[b];
    } else {
      const unsigned long long seed = (unsigned long long)p.seed[0];
      const int R = p.R > 1 ? p.R : 1, sq = b / R;
      ORION_DASSERT(sq * R < p.B);
      const unsigned x0 = sp_philox_x0((unsigned)(p.positions[sq] + p.pos_off + (b - sq * R)), (unsigned)sq, 0u, 0u,
                                       (unsigned)seed, (unsigned)(seed >> 32));
      // rounded to fp32; the largest word's sum is a tie that rounds to 1.0, hence the cap
      u = fminf((float)(x0 >> 8) * 0x1p-24f + 0x1p-25f, 0x1.fffffep-1f);
    }
    s_u = u;
    if (p.u_out) p.u_out[b] = u;
    s_max = 0;
    s_first = INT_MAX;
    s_last = s_lastw = -1;
  }
  for (int i = tid; i < 256 * SP_COPIES; i += SP_NT) hist[i] = 0;
  if constexpr (STAGED) {
    ORION_DASSERT(nslots <= SP_STAGE_SLOTS);
    for (int j = tid; j < nslots; j += SP_NT) sm[j] = sp_load_slot(row, a, V, j);
  }
  __syncthreads();

  auto slot = [&](int j) -> u32x4 {
    ORION_DASSERT(j >= 0 && j < nslots);
    if constexpr (STAGED) return sm[j];
    else return sp_load_slot(row, a, V, j);
  };

  // ---- the row's largest key, and the histogram of the high byte
  const int copy = lane & (SP_COPIES - 1);
  unsigned mx = 0;
  for (int j = j0; j < j1; ++j) {
    const u32x4 s = slot(j);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned k = sp_elem(s, e);
      if (k != SP_NONE) {
        mx = k > mx ? k : mx;
        if (select) atomicAdd(&hist[(k >> 8) * SP_COPIES + copy], 1);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned v = (unsigned)__shfl_xor((int)mx, o, 64);
    mx = v > mx ? v : mx;
  }
  if (lane == 0) atomicMax(&s_max, (int)mx);

  unsigned thr = 0;  // keep every element
  if (select) {      // block-uniform
    __syncthreads();
    if (tid < 256) {
      int c = 0;
#pragma unroll
      for (int i = 0; i < SP_COPIES; ++i) c += hist[tid * SP_COPIES + i];
      bins[tid] = c;
    }
    __syncthreads();
    for (int i = tid; i < 256 * SP_COPIES; i += SP_NT) hist[i] = 0;
    if (wv == 0) sp_pick_digit(bins, top_k, lane, pick);
    __syncthreads();
    const unsigned d1 = (unsigned)pick[0];
    const int krem = pick[1];
    ORION_DASSERT(d1 < 256 && krem >= 1);
    for (int j = j0; j < j1; ++j) {
      const u32x4 s = slot(j);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned k = sp_elem(s, e);
        if (k != SP_NONE && (k >> 8) == d1) atomicAdd(&hist[(k & 255u) * SP_COPIES + copy], 1);
      }
    }
    __syncthreads();
    if (tid < 256) {
      int c = 0;
#pragma unroll
      for (int i = 0; i < SP_COPIES; ++i) c += hist[tid * SP_COPIES + i];
      bins[tid] = c;
    }
    __syncthreads();
    if (wv == 0) sp_pick_digit(bins, krem, lane, pick);
    __syncthreads();
    ORION_DASSERT(pick[0] >= 0 && pick[0] < 256);
    thr = (d1 << 8) | (unsigned)pick[0];
  } else {
    __syncthreads();
  }

  // ---- weights: this thread's range in index order
  const float zmax = sp_value((unsigned)s_max) / t;
  float S = 0.f;
  int last = -1, lastw = -1;  // last kept index, last one of positive weight
  for (int j = j0; j < j1; ++j) {
    const u32x4 s = slot(j);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned k = sp_elem(s, e);
      if (k >= thr && k != SP_NONE) {
        const float w = __expf(sp_value(k) / t - zmax);
        S += w;
        last = (int)(8L * j + e - a);
        if (w > 0.f) lastw = last;
      }
    }
  }
  float inc = S;  // inclusive scan over the wave, lane order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  float before = __shfl_up(inc, 1, 64);
  if (lane == 0) before = 0.f;
  if (lane == 63) wtot[wv] = inc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int v = __shfl_xor(last, o, 64), vw = __shfl_xor(lastw, o, 64);
    last = v > last ? v : last;
    lastw = vw > lastw ? vw : lastw;
  }
  if (lane == 0) {
    atomicMax(&s_last, last);
    atomicMax(&s_lastw, lastw);
  }
  __syncthreads();
  float base = 0.f, Z = 0.f;
#pragma unroll
  for (int i = 0; i < SP_NW; ++i) {  // wave order
    if (i == wv) base = Z;
    Z += wtot[i];
  }
  const float excl = base + before, target = s_u * Z;
  // `excl` comes from the scan tree, the sum the previous thread tested from another association
  // of the same terms: they can differ by an ulp, so a target between the two reaches a thread
  // whatever it owns.  Only a thread with weight of its own may claim it (its walk then ends on
  // a token, the same additions); a target no such thread exceeds takes the exit below.  False
  // throughout for a NaN sum.
  const bool cross = S > 0.f && excl + S > target;
  const unsigned long long m = __ballot(cross);
  if (m != 0 && lane == __ffsll((long long)m) - 1) atomicMin(&s_first, tid);
  __syncthreads();

  long tok = -1;
  if (s_first == tid) {
    float run = 0.f;
    for (int j = j0; j < j1 && tok < 0; ++j) {
      const u32x4 s = slot(j);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned k = sp_elem(s, e);
        if (tok < 0 && k >= thr && k != SP_NONE) {
          const float w = __expf(sp_value(k) / t - zmax);
          run += w;
          if (w > 0.f && excl + run > target) tok = 8L * j + e - a;  // never an entry of weight 0
        }
      }
    }
    ORION_DASSERT(tok >= 0);
  } else if (s_first == INT_MAX && tid == 0) {
    tok = s_lastw >= 0 ? s_lastw : (s_last > 0 ? s_last : 0);
  }
  if (tok >= 0) {
    ORION_DASSERT(tok < V);
    p.out_tokens[(long)b * p.out_s] = tok;
    if (p.history) {
      const int pos = p.positions[b];
      if (pos >= 0 && pos < p.L) p.history[(long)b * p.history_rs + pos] = tok;
    }
  }
}

}  // namespace orion

using namespace orion;

// No allocation, synchronisation or copy: the launch is captured into the decode step's graph.
int orion_sample_tokens(const SampleParams& p, hipStream_t st) {
  if (p.B < 1 || p.V < 1) return -1;
  if (!p.logits || !p.params || !p.out_tokens) return -2;
  if (!p.u && (!p.seed || !p.positions)) return -3;
  if (p.history && (!p.positions || p.L < 1 || p.R > 1)) return -4;
  if (p.R < 0 || (p.R > 1 && p.B % p.R)) return -1;
  const long nslots = ((long)p.V + 7 + 7) / 8;  // the most slots a row of V can take (a <= 7)
  if (nslots <= SP_STAGE_SLOTS) {
    constexpr int lds = SP_STAGE_SLOTS * 16;
    if (dynamic_lds_once<sample_kernel<true>>(lds) != hipSuccess) return -5;
    sample_kernel<true><<<p.B, SP_NT, (size_t)nslots * 16, st>>>(p);
  } else {
    sample_kernel<false><<<p.B, SP_NT, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}
