// The device-side pieces of a speculative decode step on gfx950 besides the model's forward: the
// n-gram draft and the accept rule.  Both read their per-token state (the current column, the
// lengths, the stop columns) from device memory, so their launches sit inside a captured step.
//
// spec_draft_kernel, grid B, 256 threads: out[b, 0] = history[b, cur[b]]; the k drafts continue the
//   latest earlier occurrence of the row's last g tokens: j = the largest index in [0, cur - g] with
//   history[b, j + i] == history[b, cur - g + 1 + i] for all i < g (the threads scan the candidates
//   256 at a time and meet in an integer LDS max, which no order changes), P = cur - g + 1 - j, and
//   draft i = history[b, j + g + ((i - 1) mod P)]: the continuation, periodic once it runs into
//   the present.  Without a match (or cur < g) every draft is history[b, cur].
// spec_accept_kernel, one thread per row: a = the number of leading drafts tokens[b, i] (i = 1..k)
//   that equal target[b, i - 1]; e = clamp(min(a + 1, stop[b] - start[b]), 0, k + 1) tokens are
//   emitted: history[b, start[b] + 1 + i] = target[b, i] for i < e (columns >= L skipped) and
//   lens[b] = start[b] + e.  Nothing else is written.
#include "common.h"
#include "launchers.h"

namespace orion {

__global__ __launch_bounds__(256) void spec_draft_kernel(const long* __restrict__ history, long hist_rs,
                                                         const int* __restrict__ cur_col, long* __restrict__ out,
                                                         long out_rs, int B, int L, int k1, int g) {
  __shared__ int best;
  const int b = blockIdx.x, tid = threadIdx.x;
  ORION_DASSERT(b < B);
  const long* h = history + (long)b * hist_rs;
  int cur = cur_col[b];
  cur = cur < 0 ? 0 : (cur > L - 1 ? L - 1 : cur);  // a column of the row whatever the caller's state
  if (tid == 0) best = -1;
  __syncthreads();
  const int tail = cur - g + 1;  // the first of the last g tokens
  for (int j = tid; j < tail; j += 256) {  // j <= cur - g; no candidate when cur < g
    bool same = true;
    for (int i = 0; i < g && same; ++i) {
      ORION_DASSERT(j + i >= 0 && tail + i <= cur && cur < L);
      same = h[j + i] == h[tail + i];
    }
    if (same) atomicMax(&best, j);
  }
  __syncthreads();
  const int j = best;
  for (int i = tid; i < k1; i += 256) {
    int col = cur;
    if (i > 0 && j >= 0) col = j + g + (i - 1) % (tail - j);
    ORION_DASSERT(col >= 0 && col <= cur && cur < L);
    out[(long)b * out_rs + i] = h[col];
  }
}

__global__ __launch_bounds__(64) void spec_accept_kernel(const long* __restrict__ tokens, long tok_rs,
                                                         const long* __restrict__ target, long tgt_rs,
                                                         const int* __restrict__ start, int* __restrict__ lens,
                                                         const int* __restrict__ stop, long* __restrict__ history,
                                                         long hist_rs, int B, int k, int L) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const long* tok = tokens + (long)b * tok_rs;
  const long* tgt = target + (long)b * tgt_rs;
  int a = 0;
  while (a < k && tok[a + 1] == tgt[a]) ++a;
  const long s = start[b];
  long e = (long)stop[b] - s;
  e = e < a + 1 ? e : a + 1;
  e = e < 0 ? 0 : (e > k + 1 ? k + 1 : e);
  ORION_DASSERT(a <= k && e >= 0 && e <= k + 1);  // tok[1..a + 1) and tgt[0..e) lie in rows of k + 1
  for (int i = 0; i < (int)e; ++i) {
    const long col = s + 1 + i;
    if (col >= 0 && col < L) history[(long)b * hist_rs + col] = tgt[i];
  }
  lens[b] = (int)(s + e);
}

}  // namespace orion

using namespace orion;

// No allocation, synchronisation or copy: both launches are captured into the decode step's graph.
int orion_spec_draft(const long* history, long hist_rs, const int* cur, long* out, long out_rs, int B, int L,
                     int k1, int ngram, hipStream_t st) {
  if (B < 1 || L < 1 || k1 < 1 || ngram < 1) return -1;
  if (!history || !cur || !out) return -3;
  spec_draft_kernel<<<B, 256, 0, st>>>(history, hist_rs, cur, out, out_rs, B, L, k1, ngram);
  return (int)hipGetLastError();
}

int orion_spec_accept(const long* tokens, long tok_rs, const long* target, long tgt_rs, const int* start,
                      int* lens, const int* stop, long* history, long hist_rs, int B, int k, int L,
                      hipStream_t st) {
  if (B < 1 || k < 0 || L < 1) return -1;
  if (!tokens || !target || !start || !lens || !stop || !history) return -3;
  spec_accept_kernel<<<(B + 63) / 64, 64, 0, st>>>(tokens, tok_rs, target, tgt_rs, start, lens, stop, history,
                                                  hist_rs, B, k, L);
  return (int)hipGetLastError();
}
