"""csrc/sample.hip through ``ops.sample_tokens`` against the fp64 reference: the planted V = 1000
fixture (exact membership, counts, the fp64 CDF bracket), planted entries on both sides of the
kernel's thread and wave range boundaries at ragged shapes and strides (exact tokens), its Philox
uniforms bit for bit, the token / history outputs, reproducibility and the argument checks."""
import pytest
import torch

from orion_amd import ops
from orion_amd.ops import reference as ref
from orion_amd.ops.decode import sample_params
from sample_fixtures import boundary_case, check_brackets, check_planted_counts, planted_batch, planted_row

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_planted_fixture_through_the_kernel():
    logits, u, p = planted_batch()
    dl, du = logits.to(DEV), u.to(DEV)
    assert ops.sample_tokens_eligible(dl)
    tok = ops.sample_tokens(dl, 1.0, 8, u=du)
    assert tok.shape == (512, 1) and tok.dtype == torch.int64 and tok.is_cuda
    check_planted_counts(tok.cpu(), p)
    check_brackets(logits, 1.0, 8, tok.cpu(), u)
    assert torch.equal(tok.cpu(), ops.sample_tokens(logits, 1.0, 8, u=u))  # the reference's tokens
    assert torch.equal(tok, ops.sample_tokens(dl, 1.0, 8, u=du))           # a second launch
    # without top-k the whole row is kept: the bracket alone decides
    tok = ops.sample_tokens(dl, 0.8, None, u=du)
    check_brackets(logits, 0.8, None, tok.cpu(), u)
    assert torch.equal(tok, ops.sample_tokens(dl, 0.8, None, u=du))
    # the stock-op composition (fp32 logits) follows the same rule on the same u
    check_brackets(logits, 1.0, 8, ops.sample_tokens(dl.float(), 1.0, 8, u=du).cpu(), u)


# (B, V, extra row stride, first column of the slice): contiguous rows, a column slice of a wider
# NaN-filled buffer, and odd V with an odd row stride (rows at every 2-byte alignment)
SHAPES = [(B, V, 0, 0) for V in (1, 7, 257, 50257, 50304) for B in (1, 16)]
SHAPES += [(16, 257, 24, 8), (16, 50257, 14, 5), (16, 50304, 13, 5), (16, 7, 2, 1), (3, 66001, 0, 0)]


@pytest.mark.parametrize("B,V,pad,col0", SHAPES)
@pytest.mark.parametrize("top_k", [None, 32])
def test_planted_entries_at_the_range_boundaries(B, V, pad, col0, top_k):
    """66001 is past the rows staged in LDS: the passes read the row from memory."""
    logits, u, targets = boundary_case(B, V, DEV, pad, col0)
    tok = ops.sample_tokens(logits, 1.0, top_k, u=u)
    assert tok.flatten().tolist() == targets.tolist()
    assert torch.equal(tok.cpu(), ops.sample_tokens(logits.cpu(), 1.0, top_k, u=u.cpu()))


def test_ties_and_edge_settings_through_the_kernel():
    row = torch.linspace(-4.0, 1.0, 64)
    row[[5, 40]] = torch.tensor([5.0, 4.0])
    row[[0, 9, 31, 32, 63]] = 3.0
    rows = row.to(torch.bfloat16).repeat(256, 1)
    u = (torch.arange(256, dtype=torch.float32) + 0.5) / 256
    tok = ops.sample_tokens(rows.to(DEV), 1.0, 3, u=u.to(DEV)).cpu()
    assert set(tok.flatten().tolist()) == {0, 5, 9, 31, 32, 40, 63}
    check_brackets(rows, 1.0, 3, tok, u)
    big = planted_row().repeat(4, 1)
    us = torch.tensor([0.001, 0.3, 0.77, 0.999])
    for t, k in ((1.0, 1), (1e-6, None), (0.0, None), (-1.0, 200)):
        assert ops.sample_tokens(big.to(DEV), t, k, u=us.to(DEV)).flatten().tolist() == [0] * 4, (t, k)
    want = ops.sample_tokens(big, 0.9, None, u=us)
    for k in (0, 1000, 2 ** 31 - 1):
        assert torch.equal(ops.sample_tokens(big.to(DEV), 0.9, k, u=us.to(DEV)).cpu(), want)
    two = torch.tensor([[0.0, 1e-6]], dtype=torch.bfloat16, device=DEV)
    for t in (1e-6, 1e-9):  # clamped to 1e-6, not used as it is: p = 0.27 / 0.73
        assert int(ops.sample_tokens(two, t, None, u=torch.tensor([0.1], device=DEV))) == 0
        assert int(ops.sample_tokens(two, t, None, u=torch.tensor([0.5], device=DEV))) == 1
    # rows of -inf, NaN and -0 / +0 ties: the choice is unspecified or plain, the range is not
    odd = torch.zeros(4, 777, dtype=torch.bfloat16)
    odd[0] = float("-inf")
    odd[1, 100] = float("nan")
    odd[2] = float("nan")
    odd[3, ::2] = -0.0
    for k in (None, 5):
        tok = ops.sample_tokens(odd.to(DEV), 1.0, k, u=us.to(DEV)).cpu()
        assert int(tok.min()) >= 0 and int(tok.max()) < 777
        assert int(tok[3]) == int(ops.sample_tokens(odd[3:], 1.0, k, u=us[3:]))  # -0 ties with +0: all kept


def test_kernel_uniforms_history_and_out():
    B, V, L = 16, 257, 40
    logits = boundary_case(B, V, DEV)[0]
    pos = torch.tensor([0, 1, 39, 40, 41, 7, 7, 2 ** 31 - 1, 12, 5, 38, 3, 3, 3, 100, 20], dtype=torch.int32).to(DEV)
    seed = torch.tensor([-0x1234567890abcdef], dtype=torch.int64, device=DEV)
    hist = torch.full((B, L), -7, dtype=torch.long, device=DEV)
    out = torch.full((B,), -7, dtype=torch.long, device=DEV)
    u_out = torch.zeros(B, device=DEV)
    tok = ops.sample_tokens(logits, 1.0, 32, seed=seed, positions=pos, out=out, history=hist, u_out=u_out)
    want_u = ref.philox_uniform(seed, pos)
    assert torch.equal(u_out, want_u)  # bit for bit
    assert torch.equal(u_out.cpu(), ref.philox_uniform(int(seed), pos.cpu()))
    assert tok.shape == (B, 1) and tok.data_ptr() == out.data_ptr()
    assert torch.equal(tok.cpu(), ops.sample_tokens(logits.cpu(), 1.0, 32, u=want_u.cpu()))
    expect = torch.full((B, L), -7, dtype=torch.long)
    for b, p in enumerate(pos.tolist()):
        if p < L:
            expect[b, p] = int(tok[b])
    assert torch.equal(hist.cpu(), expect)  # positions >= L wrote nothing
    # an int seed and a (B, 1) out of a wider buffer; two launches agree
    wide = torch.full((B, 3), -7, dtype=torch.long, device=DEV)
    again = ops.sample_tokens(logits, 1.0, 32, seed=int(seed), positions=pos, out=wide[:, 1:2])
    assert torch.equal(again, tok) and torch.equal(wide[:, 1:2], tok) and bool((wide[:, ::2] == -7).all())
    # device-resident parameters: the same launch arguments, another setting
    params = sample_params(1.0, 32, DEV)
    a = ops.sample_tokens(logits, params=params, u=u_out)
    sample_params(1.0, 1, out=params)
    b = ops.sample_tokens(logits, params=params, u=u_out)
    assert torch.equal(a, tok) and not torch.equal(b, tok)
    assert torch.equal(b.cpu(), ops.sample_tokens(logits.cpu(), 1.0, 1, u=u_out.cpu()))
    assert bool((logits.gather(1, b) == 8.0).all())  # top-k 1 keeps the ties at the maximum, nothing else


def test_argument_checks():
    ops.load_ext(required=True)
    logits = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    u = torch.full((4,), 0.5, device=DEV)
    C = torch.ops.orion_amd.sample_tokens
    params = sample_params(1.0, None, DEV)
    seed = torch.zeros(1, dtype=torch.int64, device=DEV)
    C(logits, params, u, None, None)
    C(logits, params, None, seed, pos)
    for bad in (
        lambda: C(logits, params, None, seed, pos.cpu()),                    # positions on the host
        lambda: C(logits, params, None, seed.cpu(), pos),                    # seed on the host
        lambda: C(logits, params.cpu(), u, None, None),                      # parameters on the host
        lambda: C(logits, params, None, seed, pos.long()),                   # wrong dtypes
        lambda: C(logits, params, u.double(), None, None),
        lambda: C(logits.float(), params, u, None, None),
        lambda: C(logits, params.float(), u, None, None),
        lambda: C(logits, params, u, None, None, torch.zeros(4, 1, dtype=torch.int32, device=DEV)),
        lambda: C(torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV)[:, ::2], params, u, None, None),  # inner stride
        lambda: C(logits, params, u[:3], None, None),                        # shapes
        lambda: C(logits, params, None, None, pos),                          # no u and no seed
        lambda: C(logits, params, u, None, None, None, torch.zeros(4, 8, dtype=torch.long, device=DEV)),  # no positions
        lambda: C(logits, params, u, None, pos, None, torch.zeros(8, 4, dtype=torch.long, device=DEV).t()),
    ):
        with pytest.raises(RuntimeError):
            bad()
    assert not ops.sample_tokens_eligible(logits.float()) and not ops.sample_tokens_eligible(logits.cpu())


def test_every_row_gets_a_token_at_thread_boundaries_followed_by_empty_threads():
    """The sum a thread is handed as "before my range" comes from the wave's scan tree, the sum
    its predecessor tested from another association of the same terms; the two can differ by an
    ulp.  A target between them must not be claimed by a thread that owns no kept entry (it
    would find no token and store none).  32 rows of logits with kept entries in threads 0, 1, 2
    and 100 only (V 1024: a thread owns 8 entries), each under the 512 consecutive fp32 u around
    the end of thread 2's range, cover that gap wherever the three weights open it; every row
    must store a token of the kept set inside the fp64 bracket.  A u <= 0 is the same hole at
    thread 0 and takes the first kept entry."""
    V, CFG, NU, kept = 1024, 32, 512, [3, 8, 16, 800]
    g = torch.Generator().manual_seed(7)
    base = (torch.randn(CFG, V, generator=g) * 0.5 - 30.0).to(torch.bfloat16)
    vals = 7.0 + torch.randint(0, 127, (CFG, 4), generator=g).float() / 128  # bf16 steps in [7, 8)
    vals[:, 0] = 8.0
    base[:, kept] = vals.to(torch.bfloat16)
    c, Z = ref.sample_cdf(base, 1.0, 4)
    edge = (c[:, 16] / Z[:, 0]).float()  # mass through thread 2's entry
    bits = edge.view(torch.int32)[:, None] + torch.arange(-NU // 2, NU // 2, dtype=torch.int32)[None]
    u = bits.view(torch.float32).reshape(-1)
    logits = base[:, None, :].expand(CFG, NU, V).reshape(-1, V).contiguous()
    out = torch.full((CFG * NU, 1), -7, dtype=torch.long, device=DEV)
    ops.sample_tokens(logits.to(DEV), 1.0, 4, u=u.to(DEV), out=out)
    tok = out.cpu()
    assert int((tok == -7).sum()) == 0, f"{int((tok == -7).sum())} rows stored no token"
    assert set(tok.flatten().tolist()) <= set(kept)
    check_brackets(logits, 1.0, 4, tok, u)
    out.fill_(-7)
    ops.sample_tokens(logits[:4].to(DEV), 1.0, 4, u=torch.tensor([-1.0, -1e-30, 0.0, -0.0], device=DEV), out=out[:4])
    assert out[:4].flatten().tolist() == [3] * 4
