"""The draft and accept kernels (csrc/spec_decode.hip) and the sampler's rows per sequence
(csrc/sample.hip) on the GPU, integer-exact against the references and the hand-worked cases."""
import pytest
import torch

from orion_amd import ops
from orion_amd.ops import reference as ref
from sample_fixtures import check_planted_counts, planted_batch
from spec_fixtures import K, accept_case, draft_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", sorted(draft_cases()))
def test_draft_kernel_on_hand_cases(name):
    history, cur, g, want = draft_cases()[name]
    out = torch.full((history.shape[0], K + 1), -1, dtype=torch.int64, device=DEV)
    dh = history.to(DEV)
    ops.spec_draft(dh, cur.to(DEV), out, g)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out.cpu(), ref.spec_draft(history, cur, torch.zeros_like(want), g))
    assert torch.equal(dh.cpu(), history)


@pytest.mark.parametrize("g", [1, 3])
def test_draft_kernel_against_the_reference_on_repetitive_rows(g):
    """Rows over a 5-token alphabet (matches everywhere, the latest must win), a different cur per
    row, L = 700, k = 7; out is a column slice of a wider buffer."""
    gen = torch.Generator().manual_seed(g)
    history = torch.randint(0, 5, (6, 700), generator=gen)
    cur = torch.tensor([0, 2, 3, 255, 513, 699], dtype=torch.int32)
    wide = torch.full((6, 11), -1, dtype=torch.int64, device=DEV)
    ops.spec_draft(history.to(DEV), cur.to(DEV), wide[:, 2:10], g)
    want = ref.spec_draft(history, cur, torch.zeros(6, 8, dtype=torch.int64), g)
    assert torch.equal(wide[:, 2:10].cpu(), want)
    assert bool((wide[:, :2] == -1).all()) and bool((wide[:, 10:] == -1).all())


def test_accept_kernel_on_hand_cases():
    tokens, target, start, stop, L, want_e, want_hist = accept_case()
    history = torch.full((tokens.shape[0], L), -1, dtype=torch.int64, device=DEV)
    lens = (start + 4).to(DEV)
    dstart, dstop = start.to(DEV), stop.to(DEV)
    ops.spec_accept(tokens.to(DEV), target.to(DEV), dstart, lens, dstop, history)
    assert torch.equal(history.cpu(), want_hist)  # only columns [start + 1, start + e] changed
    assert lens.cpu().tolist() == [int(s) + e for s, e in zip(start, want_e)]
    assert torch.equal(dstart.cpu(), start) and torch.equal(dstop.cpu(), stop)
    rh, rl = torch.full((tokens.shape[0], L), -1, dtype=torch.int64), start + 4
    ref.spec_accept(tokens, target, start, rl, stop, rh)
    assert torch.equal(history.cpu(), rh) and torch.equal(lens.cpu(), rl)


def test_accept_kernel_against_the_reference_on_random_rows():
    gen = torch.Generator().manual_seed(0)
    B, k, L = 16, 7, 40
    target = torch.randint(0, 3, (B, k + 1), generator=gen)
    tokens = torch.randint(0, 3, (B, k + 1), generator=gen)
    tokens[::2, 1:4] = target[::2, :3]  # a >= 3 on every other row
    start = torch.randint(0, L, (B,), generator=gen).to(torch.int32)
    stop = start + torch.randint(-2, 12, (B,), generator=gen).to(torch.int32)
    history = torch.full((B, L + 3), -1, dtype=torch.int64, device=DEV)[:, :L]  # a row stride of L + 3
    lens = (start + k + 1).to(DEV)
    ops.spec_accept(tokens.to(DEV), target.to(DEV), start.to(DEV), lens, stop.to(DEV), history)
    rh, rl = torch.full((B, L), -1, dtype=torch.int64), start + k + 1
    ref.spec_accept(tokens, target, start, rl, stop, rh)
    assert torch.equal(history.cpu(), rh) and torch.equal(lens.cpu(), rl)


def test_sampler_rows_per_seq_equals_plain_calls_per_position():
    B, R, V = 3, 4, 1001
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(B * R, V, generator=gen).to(torch.bfloat16).to(DEV)
    pos = torch.tensor([5, 0, 17], dtype=torch.int32, device=DEV)
    out = torch.full((B, R), -1, dtype=torch.int64, device=DEV)
    u = torch.zeros(B * R, device=DEV)
    got = ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, out=out.view(-1), rows_per_seq=R,
                            position_offset=1, u_out=u)
    assert torch.equal(got.view(B, R), out)
    assert torch.equal(u.cpu(), ref.philox_uniform(99, pos.cpu(), R, 1))
    for t in range(R):
        want = ops.sample_tokens(logits[t::R], 0.8, 40, seed=99, positions=pos + 1 + t)
        assert torch.equal(out[:, t:t + 1], want), t
    with pytest.raises((ValueError, RuntimeError)):
        ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, rows_per_seq=R,
                          history=torch.zeros(B * R, 8, dtype=torch.long, device=DEV))
    with pytest.raises((ValueError, RuntimeError)):
        ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, rows_per_seq=5)


def test_sampler_defaults_are_unchanged():
    """The planted fixture through the kernel as before, and the explicit defaults are the op
    without the keywords (Philox path, history included)."""
    logits, u, p = planted_batch()
    tok = ops.sample_tokens(logits.to(DEV), 1.0, 8, u=u.to(DEV))
    check_planted_counts(tok.cpu(), p)
    assert torch.equal(tok, ops.sample_tokens(logits.to(DEV), 1.0, 8, u=u.to(DEV), rows_per_seq=1, position_offset=0))
    rows = logits[:4].to(DEV)
    pos = torch.tensor([3, 1, 4, 1], dtype=torch.int32, device=DEV)
    h1 = torch.zeros(4, 6, dtype=torch.long, device=DEV)
    h2 = torch.zeros_like(h1)
    a = ops.sample_tokens(rows, 1.0, 8, seed=7, positions=pos, history=h1)
    b = ops.sample_tokens(rows, 1.0, 8, seed=7, positions=pos, history=h2, rows_per_seq=1, position_offset=0)
    assert torch.equal(a, b) and torch.equal(h1, h2)
    assert torch.equal(h1.gather(1, pos.long().view(4, 1)), a)
