"""Inputs shared by the sampling tests (tests/test_sample_cpu.py, tests/test_sample_gpu.py):
the V = 1000 row with eight planted entries, fp64 CDF helpers, and the index ranges of
csrc/sample.hip's threads."""
import torch

from orion_amd.ops import reference as ref

PLANTED = (0, 1, 63, 64, 255, 256, 511, 999)
ROWS = 512


def planted_row(V=1000):
    """randn under a fixed seed clamped to <= 2, with logits 8.0, 7.75, ..., 6.25 at PLANTED (bf16
    holds all of them exactly): with T = 1 and top_k = 8 exactly the planted entries are kept and
    the least likely has p = 0.044."""
    g = torch.Generator().manual_seed(1234)
    row = torch.randn(V, generator=g).clamp_(max=2.0)
    row[list(PLANTED)] = 8.0 - 0.25 * torch.arange(len(PLANTED), dtype=torch.float32)
    return row.to(torch.bfloat16)


def planted_batch():
    """(logits (512, 1000) bf16, u (512,) fp32 with u_i = (i + 0.5) / 512, fp64 p of PLANTED)."""
    row = planted_row()
    u = ((torch.arange(ROWS, dtype=torch.float64) + 0.5) / ROWS).float()
    p = torch.softmax(row[list(PLANTED)].double(), dim=0)
    return row.repeat(ROWS, 1), u, p


def check_planted_counts(tokens, p):
    """Every token is a planted index, and index j is drawn 512 p_j +- 1 times: the u are an even
    grid, so the count of an interval of length p is within one of 512 p."""
    toks = tokens.reshape(-1).tolist()
    assert set(toks) <= set(PLANTED), sorted(set(toks) - set(PLANTED))
    for j, pj in zip(PLANTED, p.tolist()):
        n = toks.count(j)
        assert abs(n - ROWS * pj) <= 1.0, (j, n, ROWS * pj)


def brackets(logits, temperature, top_k, tokens):
    """fp64 probability mass before and through each row's token: (lo, hi), each (B,)."""
    c, Z = ref.sample_cdf(logits.cpu(), temperature, top_k)
    c = torch.cat((torch.zeros_like(Z), c), dim=1) / Z
    t = tokens.reshape(-1, 1).cpu()
    return c.gather(1, t)[:, 0], c.gather(1, t + 1)[:, 0]


def check_brackets(logits, temperature, top_k, tokens, u):
    """P64(prefix before token) - tol <= u <= P64(prefix through token) + tol with tol =
    2 (V + 8) 2^-24, the bound of any fp32 summation order of V positive terms applied to the
    numerator and the denominator; the token also lies in the exact kept set."""
    V = logits.shape[1]
    tol = 2 * (V + 8) * 2.0 ** -24
    lo, hi = brackets(logits, temperature, top_k, tokens)
    ud = u.double().cpu()
    keep = ref.sample_keep_mask(logits.cpu(), top_k)
    assert bool(keep.gather(1, tokens.reshape(-1, 1).cpu()).all()), "a token outside the kept set"
    bad = ~((lo - tol <= ud) & (ud <= hi + tol))
    assert not bool(bad.any()), (bad.nonzero().flatten().tolist()[:8], lo[bad][:4], ud[bad][:4], hi[bad][:4], tol)


def midpoint_u(row, temperature, top_k, index):
    """The u at the middle of ``index``'s CDF interval of one row (V,), fp32."""
    lo, hi = brackets(row[None], temperature, top_k, torch.tensor([index]))
    return float(((lo + hi) / 2).float())


# ---- the layout of csrc/sample.hip: 1024 threads, thread t owns `cs` slots of 8 elements in
# coordinates aligned to 16 bytes (element i sits at a + i), cs odd
THREADS = 1024


def thread_range_starts(ptr, V):
    """Row indices at which a thread's range starts (a new wave's every 64th), for a row at
    byte address ``ptr``."""
    a = (ptr % 16) // 2
    nslots = (a + V + 7) // 8
    cs = ((nslots + THREADS - 1) // THREADS) | 1
    return [8 * cs * t - a for t in range(1, THREADS) if 0 < 8 * cs * t - a < V]


def plant_indices(ptr, V):
    """First and last index, both sides of the first two thread boundaries, of every wave boundary
    up to the fourth, and of the last thread boundary of the row."""
    starts = thread_range_starts(ptr, V)
    pick = starts[:2] + starts[63::64][:4] + starts[-1:]
    idx = {0, V - 1}
    for s in pick:
        idx |= {s - 1, s}
    return sorted(i for i in idx if 0 <= i < V)


def boundary_case(B, V, device, stride_pad=0, col0=0):
    """logits (B, V) bf16 -- a column slice from ``col0`` of a NaN-filled (B, V + stride_pad)
    buffer when either is set -- with a background near -30 and entries 8.0 / 7.75 / 7.5 / 7.25
    at each row's :func:`plant_indices`; row r targets its (r mod n)-th planted entry.  Returns
    (logits, u (B,) fp32 at the middle of the target's CDF interval, targets (B,)).  The
    background's whole mass is below 1e-11 of the planted entries', so the expected token is the
    target with or without a top-k above the 16 entries a row can have planted."""
    g = torch.Generator().manual_seed(V)
    wide = torch.full((B, V + stride_pad), float("nan"), dtype=torch.bfloat16, device=device)
    logits = wide[:, col0:col0 + V]
    assert logits.stride(0) == V + stride_pad
    host = (torch.randn(B, V, generator=g) * 0.5 - 30.0).to(torch.bfloat16)
    targets = []
    for r in range(B):
        ptr = logits.data_ptr() + 2 * r * logits.stride(0) if device != "cpu" else 0
        idx = plant_indices(ptr, V)
        host[r, idx] = (8.0 - 0.25 * (torch.arange(len(idx)) % 4)).to(torch.bfloat16)
        targets.append(idx[r % len(idx)])
    logits.copy_(host)
    u = torch.tensor([midpoint_u(host[r], 1.0, None, targets[r]) for r in range(B)], dtype=torch.float32)
    return logits, u.to(device), torch.tensor(targets)
