"""The sampling rule's CPU side: ``ref.philox_uniform`` against the Philox4x32-10 known answers,
``ops.sample_tokens`` on CPU tensors (the fp64 reference and oracle of tests/test_sample_gpu.py)
on the planted V = 1000 fixture, on ties at the top-k threshold and on the edge settings, and
``generate(use_cache="fused", sampler="device")`` of both models."""
import numpy as np
import pytest
import torch

from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from sample_fixtures import check_brackets, check_planted_counts, midpoint_u, planted_batch, planted_row

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in ref.philox4x32_10(np.array(counter, dtype=np.uint64), key)) == want


def test_philox_uniform_is_word_zero_of_the_counter_and_inside_the_unit_interval():
    # counter (0, 0, 0, 0), key 0: the first known answer's word 0
    u = ref.philox_uniform(0, torch.zeros(1, dtype=torch.int32))
    assert u.dtype == torch.float32 and float(u[0]) == (0x6627e8d5 >> 8) * 2.0 ** -24 + 2.0 ** -25
    # a 64-bit seed is split into (low, high) key words, the counter is (position, row, 0, 0)
    seed = (0x299f31d0 << 32) | 0xa4093822
    pos = torch.tensor([7, 2 ** 31 - 1, 0], dtype=torch.int32)
    u = ref.philox_uniform(seed, pos)
    for b, p in enumerate(pos.tolist()):
        x0 = int(ref.philox4x32_10(np.array([p, b, 0, 0]), (0xa4093822, 0x299f31d0))[0])
        assert float(u[b]) == float(np.float32((x0 >> 8) * 2.0 ** -24) + np.float32(2.0 ** -25))  # rounded once
    assert torch.equal(u, ref.philox_uniform(torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed]), pos))
    many = ref.philox_uniform(-12345, torch.arange(4096, dtype=torch.int32) % 61)
    assert float(many.min()) > 0.0 and float(many.max()) < 1.0 and many.unique().numel() > 4000
    # the extremes of the map itself
    lo, hi = ref.uniform_from_word(np.array([0, 0xffffffff], dtype=np.uint32)).tolist()
    assert lo == 2.0 ** -25 and hi == 1.0 - 2.0 ** -24


def test_reference_on_the_planted_fixture():
    logits, u, p = planted_batch()
    tok = ops.sample_tokens(logits, 1.0, 8, u=u)
    assert tok.shape == (512, 1) and tok.dtype == torch.int64
    check_planted_counts(tok, p)
    check_brackets(logits, 1.0, 8, tok, u)


def _tie_row():
    row = torch.linspace(-4.0, 1.0, 64)
    row[[5, 40]] = torch.tensor([5.0, 4.0])
    row[[0, 9, 31, 32, 63]] = 3.0
    return row.to(torch.bfloat16)


def test_ties_at_the_threshold_are_all_kept():
    row = _tie_row()
    keep = ref.sample_keep_mask(row[None], 3)[0]
    assert sorted(keep.nonzero().flatten().tolist()) == [0, 5, 9, 31, 32, 40, 63]
    for j in keep.nonzero().flatten().tolist():
        u = torch.tensor([midpoint_u(row, 1.0, 3, j)])
        assert int(ops.sample_tokens(row[None], 1.0, 3, u=u)) == j
    # every u lands in the kept set
    us = (torch.arange(256, dtype=torch.float32) + 0.5) / 256
    toks = ops.sample_tokens(row.repeat(256, 1), 1.0, 3, u=us)
    assert set(toks.flatten().tolist()) == {0, 5, 9, 31, 32, 40, 63}


def test_edge_settings():
    row = planted_row()
    us = torch.tensor([0.001, 0.3, 0.77, 0.999])
    rows = row.repeat(4, 1)
    assert ops.sample_tokens(rows, 1.0, 1, u=us).flatten().tolist() == [0] * 4  # the argmax
    want = ops.sample_tokens(rows, 1.0, None, u=us)
    for k in (0, 1000, 5000):  # keep everything
        assert torch.equal(ops.sample_tokens(rows, 1.0, k, u=us), want)
    check_brackets(rows, 1.0, None, want, us)
    assert ops.sample_tokens(torch.tensor([[-3.0], [float("-inf")]], dtype=torch.bfloat16), 0.7, 5,
                             u=us[:2]).flatten().tolist() == [0, 0]  # V = 1
    # a temperature of 1e-6 or below behaves as 1e-6: the next bf16 below 8.0 is 2^-5 away, which
    # 1e-6 turns into exp(-31250) = 0, so the largest entry takes every u
    for t in (1e-6, 1e-9, 0.0, -1.0):
        assert ops.sample_tokens(rows, t, None, u=us).flatten().tolist() == [0] * 4
    # ... and not as itself: logits 1e-6 apart are z = 0 and 1 at 1e-6, p = 0.27 and 0.73
    two = torch.tensor([[0.0, 1e-6]], dtype=torch.bfloat16)
    for t in (1e-6, 1e-9, 0.0):
        assert int(ops.sample_tokens(two, t, None, u=torch.tensor([0.1]))) == 0
        assert int(ops.sample_tokens(two, t, None, u=torch.tensor([0.5]))) == 1


def test_out_history_and_philox_path():
    logits = planted_row().repeat(3, 1)
    pos = torch.tensor([4, 0, 9], dtype=torch.int32)
    hist = torch.full((3, 9), -7, dtype=torch.long)
    out = torch.zeros(3, 1, dtype=torch.long)
    u_out = torch.zeros(3)
    tok = ops.sample_tokens(logits, 1.0, 8, seed=99, positions=pos, out=out, history=hist, u_out=u_out)
    assert torch.equal(u_out, ref.philox_uniform(99, pos)) and tok.data_ptr() == out.data_ptr()
    assert torch.equal(tok, ops.sample_tokens(logits, 1.0, 8, u=u_out))
    assert hist[0, 4] == tok[0, 0] and hist[1, 0] == tok[1, 0]
    hist[0, 4] = hist[1, 0] = -7
    assert bool((hist == -7).all())  # position 9 >= L = 9 wrote nothing
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.sample_tokens(logits.float().requires_grad_(), u=u_out)


MODELS = {"gpt2-tiny": lambda: build_gpt2("gpt2-tiny"), "llama-tiny": lambda: build_llama("llama-tiny")}


@pytest.mark.parametrize("name", list(MODELS))
def test_generate_with_the_device_sampler_on_cpu(name):
    torch.manual_seed(0)
    model = MODELS[name]().eval()
    prompt = torch.randint(0, model.config.vocab_size, (2, 9))
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        outs.append(model.generate(prompt, 8, temperature=0.9, top_k=50, use_cache="fused", sampler="device"))
    assert outs[0].shape == (2, 17) and outs[0].dtype == prompt.dtype and torch.equal(outs[0][:, :9], prompt)
    assert int(outs[0].min()) >= 0 and int(outs[0].max()) < model.config.vocab_size
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    for bad in (False, True):
        with pytest.raises(ValueError, match="sampler='device'"):
            model.generate(prompt, 4, use_cache=bad, sampler="device")
    with pytest.raises(ValueError, match="sampler must be"):
        model.generate(prompt, 4, use_cache="fused", sampler="gpu")
    with pytest.raises(ValueError, match="sampler must be"):
        DecodeSession(model, 2, 32, sampler="philox")
    plain = model.decode_session(2, 32)
    assert plain.sampler == "torch" and plain.rng_seed is None and plain.sample_params is None and plain.history is None
    sess = model.decode_session(2, 32, sampler="device")
    assert sess.history.shape == (2, 33) and sess.rng_seed.shape == (1,) and sess.rng_seed.dtype == torch.int64
    # the session's draws are the oracle's: token i of row b used philox_uniform(seed, position)
    torch.manual_seed(5)
    got = sess.generate(prompt, 8, temperature=0.9, top_k=50)
    assert torch.equal(got, outs[0]) and sess.captures == 0 and sess.replays == 0
    replay = model.decode_session(2, 32)
    logits = replay.prefill(prompt)
    for i in range(8):
        pos = torch.full((2,), 9 + i, dtype=torch.int32)
        want = ref.sample_tokens(logits, 0.9, 50, seed=sess.rng_seed, positions=pos)
        assert torch.equal(want, got[:, 9 + i:10 + i]), i
        if i < 7:
            logits = replay.step(got[:, 9 + i])


def test_a_rejected_generate_leaves_the_generator_and_the_session_alone():
    torch.manual_seed(0)
    model = build_gpt2("gpt2-tiny").eval()
    sess = model.decode_session(2, 12, sampler="device")
    prompt = torch.randint(0, model.config.vocab_size, (2, 9))
    state, seed, params = torch.get_rng_state(), sess.rng_seed.clone(), sess.sample_params.clone()
    with pytest.raises(ValueError, match="overflow"):
        sess.generate(prompt, 8, temperature=0.5, top_k=3)  # 9 + 8 - 1 > 12
    assert torch.equal(sess.generate(prompt, 0), prompt)
    assert torch.equal(torch.get_rng_state(), state) and sess.cache.pos == 0
    assert torch.equal(sess.rng_seed, seed) and torch.equal(sess.sample_params, params)
