"""Inputs shared by the speculative-decoding tests (tests/test_speculative_cpu.py,
tests/test_spec_kernels_gpu.py, tests/test_speculative_gpu.py): hand-worked cases of the draft and
accept rules, corrupted draft tensors, and the step count the accept rule predicts for them."""
import torch

from orion_amd.ops import reference as ref

K = 4  # drafts per row of the draft cases


def _rows(rows, L):
    h = torch.zeros(len(rows), L, dtype=torch.int64)
    for b, r in enumerate(rows):
        h[b, :len(r)] = torch.tensor(r)
    return h


def draft_cases():
    """name -> (history (B, L) int64, cur (B,) int32, ngram, want (B, K + 1) int64), worked by hand
    from the rule: j = the latest start in [0, cur - g] of a copy of the last g tokens, P = cur - g
    + 1 - j, draft i = history[j + g + (i - 1) mod P]."""
    cases = {}
    # g = 3, rows with different cur
    cases["g3"] = (_rows([
        [1, 2, 3, 4, 5, 6, 7, 8],   # cur 7: no earlier [6, 7, 8]             -> the current token
        [5, 5, 5, 5, 5, 5, 5, 5],   # cur 2 < g: no candidate                -> the current token
        [1, 2, 3, 9, 8, 1, 2, 3],   # cur 7: [1, 2, 3] at j = 0, P = 5       -> h[3], h[4], h[5], h[6]
        [1, 2, 1, 2, 1, 2, 0, 0],   # cur 5: [2, 1, 2] at j = 1, P = 2 < K  -> h[4], h[5], h[4], h[5]
        [7, 7, 7, 7, 0, 0, 0, 0],   # cur 3 = g: the one candidate j = 0, P = 1 -> h[3] four times
    ], 12), torch.tensor([7, 2, 7, 5, 3], dtype=torch.int32), 3, torch.tensor([
        [8, 8, 8, 8, 8],
        [5, 5, 5, 5, 5],
        [3, 9, 8, 1, 2],
        [2, 1, 2, 1, 2],
        [7, 7, 7, 7, 7],
    ]))
    # g = 2, several matches: j = 0 and j = 3, the latest wins, P = 3 -> h[5], h[6], h[7], h[5]
    cases["g2_latest"] = (_rows([[1, 2, 7, 1, 2, 8, 1, 2]], 9), torch.tensor([7], dtype=torch.int32), 2,
                          torch.tensor([[2, 8, 1, 2, 8]]))
    # g = 1: token 5 (cur 8) last seen at j = 4, P = 4 -> h[5], h[6], h[7], h[8]; a row without a match
    cases["g1"] = (_rows([[3, 1, 4, 1, 5, 9, 2, 6, 5, 3], [1, 2, 3, 4, 5, 6, 7, 8, 9, 0]], 10),
                   torch.tensor([8, 8], dtype=torch.int32), 1,
                   torch.tensor([[5, 9, 2, 6, 5], [9, 9, 9, 9, 9]]))
    # L = 700 of distinct tokens, cur = 699: the only copy of the tail starts at j = 600 (g = 3) /
    # j = 650 (g = 1), which a scan by 256 threads reaches in its last iteration (j >= 512)
    for g, j in ((3, 600), (1, 650)):
        h = (torch.arange(700) + 1000).view(1, 700).clone()
        h[0, j:j + g] = h[0, 700 - g:]
        want = torch.cat((h[0, 699:], h[0, j + g:j + g + K])).view(1, K + 1)
        cases[f"long_g{g}"] = (h, torch.tensor([699], dtype=torch.int32), g, want)
    return cases


def accept_case():
    """(tokens, target (B, 4), start, stop (B,) int32, L, want_e, want_history columns) for k = 3 on
    a history of -1: a in {0, 1, k}, the cap by stop, e = 0 (stop == start and stop < start), and a
    start whose columns run past L = 12."""
    tokens = torch.tensor([[10, 1, 2, 3],    # a = 0            -> e = 1
                           [10, 7, 2, 3],    # a = 1            -> e = 2
                           [10, 7, 8, 9],    # a = 3 = k        -> e = 4
                           [10, 7, 8, 9],    # a = 3, stop = start + 2 -> e = 2
                           [10, 7, 8, 9],    # stop == start    -> e = 0
                           [10, 7, 8, 9],    # stop < start     -> e = 0
                           [10, 7, 8, 9]])   # start 9: columns 10, 11 written, 12, 13 skipped
    target = torch.tensor([[7, 8, 9, 6]] * 7)
    start = torch.tensor([4, 4, 4, 4, 4, 4, 9], dtype=torch.int32)
    stop = torch.tensor([100, 100, 100, 6, 4, 1, 100], dtype=torch.int32)
    want_e = [1, 2, 4, 2, 0, 0, 4]
    L = 12
    want_hist = torch.full((7, L), -1, dtype=torch.int64)
    for b, e in enumerate(want_e):
        for i in range(e):
            if int(start[b]) + 1 + i < L:
                want_hist[b, int(start[b]) + 1 + i] = target[b, i]
    return tokens, target, start, stop, L, want_e, want_hist


PATTERNS = ("none", "all", "third", "per_row")


def corrupt(seq, pattern, vocab):
    """``seq`` (B, L) with the tokens of the chosen positions replaced by another token: none, all,
    every third column, or a different pattern per row (row b: every (b + 2)-th column)."""
    B, L = seq.shape
    cols = torch.arange(L).view(1, L).expand(B, L)
    if pattern == "none":
        mask = torch.zeros(B, L, dtype=torch.bool)
    elif pattern == "all":
        mask = torch.ones(B, L, dtype=torch.bool)
    elif pattern == "third":
        mask = cols % 3 == 0
    else:
        mask = cols % (torch.arange(B).view(B, 1) + 2) == 0
    return torch.where(mask, (seq + 1) % vocab, seq)


def predicted_steps(seq, draft, p0, n, k):
    """(steps, emitted) of a speculative generation of n tokens from column p0 whose output is
    ``seq`` (B, p0 + n) with guesses ``draft`` (B, L) by position, by the accept rule: every draw
    up to and including the one after the last accepted guess is conditioned on a correct prefix,
    so it is seq's token; later draws do not enter the rule."""
    B, k1 = seq.shape[0], k + 1
    last = p0 + n - 1
    lens = torch.full((B,), p0, dtype=torch.int32)
    stop = torch.full((B,), last, dtype=torch.int32)
    hist = torch.zeros(B, last + 1, dtype=torch.int64)
    steps = emitted = 0
    while int(lens.min()) < last:
        start = lens.clone()
        cols = start.view(B, 1).long() + torch.arange(k1).view(1, k1)
        tokens = draft.gather(1, cols.clamp(0, draft.shape[1] - 1))
        tokens[:, 0] = seq.gather(1, cols[:, :1].clamp(max=seq.shape[1] - 1))[:, 0]
        target = seq.gather(1, (cols + 1).clamp(max=seq.shape[1] - 1))
        target[cols + 1 > last] = -1  # never emitted: past stop
        emitted += sum(ref.spec_accept(tokens, target, start, lens, stop, hist))
        steps += 1
    return steps, emitted
