"""GPU: the data kernels (ops/csrc/data.hip) bit for bit against the host oracles of tests/step_oracles.py.

The kernels' RNG is counter-based, so every output is a pure function of the arguments and each comparison
is ``torch.equal``; tests/test_step_oracles.py shows on the CPU that the oracles themselves have the right
distributions.  Shapes put L and A below, at and above the 256-thread stride, with remainders.
"""
import numpy as np
import pytest
import torch

import step_oracles as so
from proteinbert_pytorch_replication_amd.data.synthetic import CorruptionParams, SyntheticUniRefGO
from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.ops.corrupt import corrupt_batch, synth_batch, unpack_batch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 77, 1), (37, 300, 13), (5, 256, 255), (4, 512, 8943)]
SEEDS = (0, 7, 2 ** 64 - 1)
STEPS = (1, 2 ** 32 + 3)
DEFAULTS = dict(token_p=0.05, positive_p=0.25, negative_p=1e-4, blank_p=0.5)
PARAM_SETS = [DEFAULTS] + [dict(DEFAULTS, **{k: v}) for k in DEFAULTS for v in (0.0, 1.0)]


def cuda():
    return torch.device("cuda")


def length_ranges(L):
    return [(L // 2, L // 2),        # min_len == max_len
            (0, 5),                  # min_len = 0: a row of <sos><eos><pad>... is possible
            (3, L - 2),              # max_len + 2 <= L: never a crop
            (0, L - 1),              # max_len + 2 == L + 1: the crop span is 1, the start must be 0
            (0, L + 64)]             # the generator's default


def assert_synth(B, L, A, lo, hi, density, seed, step, step_dev=None, ref_step=None):
    tok, ann = synth_batch(B, L, A, lo, hi, density, seed=seed, step=step, device=cuda(), step_dev=step_dev)
    rt, ra = so.synth_batch_ref(B, L, A, lo, hi, density, seed, step if ref_step is None else ref_step)
    what = (B, L, A, lo, hi, seed, step)
    assert tok.dtype == torch.long and ann.dtype == torch.float32
    assert torch.equal(tok.cpu(), torch.from_numpy(rt)), what
    assert torch.equal(ann.cpu(), torch.from_numpy(ra)), what
    return rt, ra


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_synth_batch_bitwise(B, L, A):
    rows = set()
    for lo, hi in length_ranges(L):
        for seed in SEEDS:
            for step in STEPS:
                rt, _ = assert_synth(B, L, A, lo, hi, 0.01, seed, step)
                rows |= {"crop" if r[0] != so.SOS else "eos" if (r == so.EOS).any() else "full" for r in rt}
    assert rows >= {"crop", "eos"}                         # cropped rows and rows that end inside the window
    # the device counter is added to step: step_dev = 5 with step = 1 is step = 6
    five = torch.full((1,), 5, dtype=torch.int64, device=cuda())
    a = assert_synth(B, L, A, 0, L + 64, 0.3, 7, 1, step_dev=five, ref_step=6)
    b = assert_synth(B, L, A, 0, L + 64, 0.3, 7, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def clean_batch(B, L, A, seed):
    tok, ann = so.synth_batch_ref(B, L, A, 0, L + 64, 0.3 if A < 1000 else 0.01, seed, 1)
    flat = tok.reshape(-1)
    flat[np.nonzero(flat > so.EOS)[0][::7]] = 3            # id 3 is no residue but eligible for corruption
    return tok, ann


def assert_corrupt(tok, ann, q, seed, step, step_dev=None, ref_step=None):
    B, A = ann.shape
    params = CorruptionParams(**q)
    t_dev, a_dev = torch.from_numpy(tok).to(cuda()), torch.from_numpy(ann).to(cuda())
    X, Y, W = corrupt_batch(t_dev, a_dev, params, seed=seed, step=step, step_dev=step_dev)
    xl, xg, wl, ws = so.corrupt_batch_ref(tok, ann, q["token_p"], q["positive_p"], q["negative_p"], q["blank_p"],
                                          seed, step if ref_step is None else ref_step)
    what = (tok.shape, A, q, seed, step)
    assert torch.equal(X["local"].cpu(), torch.from_numpy(xl)), what
    assert torch.equal(X["global"].cpu(), torch.from_numpy(xg)), what
    assert torch.equal(W["local"].cpu(), torch.from_numpy(wl)), what
    assert W["global"].shape == (B, A) and (A == 1 or W["global"].stride(1) == 0)
    assert torch.equal(W["global"].cpu(), torch.from_numpy(ws)[:, None].expand(B, A)), what
    assert Y["local"] is t_dev and Y["global"] is a_dev
    assert torch.equal(t_dev.cpu(), torch.from_numpy(tok)) and torch.equal(a_dev.cpu(), torch.from_numpy(ann))
    return xl, xg, wl, ws


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_corrupt_batch_bitwise(B, L, A):
    tok, ann = clean_batch(B, L, A, seed=11)
    assert (tok == 3).any()
    for q in PARAM_SETS:
        two = False
        for seed, step in ((0, 1), (7, 2 ** 32 + 3), (2 ** 64 - 1, 1)):
            xl, xg, _, _ = assert_corrupt(tok, ann, q, seed, step)
            two |= bool((xg == 2.0).any())
        eligible = tok > so.EOS
        if q["token_p"] == 1.0:
            assert xl[eligible].min() >= 3 and (xl[eligible] != tok[eligible]).any()
        if q["token_p"] == 0.0:
            assert np.array_equal(xl, tok)
        if q["blank_p"] == 1.0 or q["positive_p"] == 1.0:
            assert not xg.any()
        if q["negative_p"] == 1.0 and B * A >= 100:
            assert two                                      # (ann + add) * keep is 2.0 where both are 1
    five = torch.full((1,), 5, dtype=torch.int64, device=cuda())
    a = assert_corrupt(tok, ann, DEFAULTS, 7, 1, step_dev=five, ref_step=6)
    b = assert_corrupt(tok, ann, DEFAULTS, 7, 6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("A", [8943, 300])
def test_corrupt_block_wide_any(A):
    """w_sample = any(ann != 0) over the whole block: one 1 per row, at the edges of every wave of the
    first stride and in the strides after it, and one row without any."""
    cols = [0, 63, 64, 191, 255, 256, A - 1]
    B = len(cols) + 1
    tok, _ = so.synth_batch_ref(B, 77, 1, 0, 141, 0.0, 3, 1)
    ann = np.zeros((B, A), np.float32)
    for b, c in enumerate(cols):
        ann[b, c] = 1.0
    for q in (DEFAULTS, dict(DEFAULTS, blank_p=1.0)):
        _, _, _, ws = assert_corrupt(tok, ann, q, 5, 1)
        assert ws.tolist() == [1.0] * len(cols) + [0.0]
    # 2.0 does not count twice and a row of the other stride only is found, too
    ann[B - 1, 300 if A > 300 else 1] = 2.0
    _, _, _, ws = assert_corrupt(tok, ann, DEFAULTS, 5, 1)
    assert ws.tolist() == [1.0] * B


def test_synthetic_generator_graph_replay():
    """SyntheticUniRefGO.next_batch() (synth, corrupt and the int64 counter add) captured once on a side
    stream, single-stream, and replayed: replay k equals the oracle at the device counter's value k."""
    B, L, A, seed = 6, 300, 517, 13
    gen = SyntheticUniRefGO(L, A, B, cuda(), density=0.01, seed=seed)
    q = DEFAULTS
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gen.next_batch()                                    # warm-up outside the capture: counter 0 -> 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(gen.step_dev.item()) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        X, Y, W = gen.next_batch()
    torch.cuda.synchronize()
    assert int(gen.step_dev.item()) == 1                   # capture records, it does not run
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(gen.step_dev.item()) == k + 1
        rt, ra = so.synth_batch_ref(B, L, A, gen.min_length, gen.max_length, gen.density, seed, 1, step_dev=k)
        xl, xg, wl, ws = so.corrupt_batch_ref(rt, ra, q["token_p"], q["positive_p"], q["negative_p"], q["blank_p"],
                                              seed, 1, step_dev=k)
        assert torch.equal(Y["local"].cpu(), torch.from_numpy(rt)), k
        assert torch.equal(Y["global"].cpu(), torch.from_numpy(ra)), k
        assert torch.equal(X["local"].cpu(), torch.from_numpy(xl)), k
        assert torch.equal(X["global"].cpu(), torch.from_numpy(xg)), k
        assert torch.equal(W["local"].cpu(), torch.from_numpy(wl)), k
        assert torch.equal(W["global"].cpu(), torch.from_numpy(ws)[:, None].expand(B, A)), k


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("L", [1, 300])
@pytest.mark.parametrize("A", [1, 7, 8, 13, 64, 8943])
def test_unpack_batch_bitwise(A, L, B):
    """Random bits with garbage in the padding bits of the last byte; through the wrapper at the exact
    byte count, and through the launcher with surplus bytes of all ones and a guard after the last row."""
    rng = np.random.default_rng(A * 1000 + L * 10 + B)
    nb = (A + 7) // 8
    bits = rng.integers(0, 256, (B, nb), dtype=np.uint8)
    if A % 8:
        bits[:, -1] |= np.uint8((0xFF << (A % 8)) & 0xFF)    # padding bits set: they must not leak
    tok = rng.integers(0, 256, (B, L), dtype=np.uint8)
    if L >= 256:
        tok[0, :256] = np.arange(256, dtype=np.uint8)      # every byte value
    rt, ra = so.unpack_ref(tok, bits, A)
    t_dev, b_dev = torch.from_numpy(tok).to(cuda()), torch.from_numpy(bits).to(cuda())
    tk, an = unpack_batch(t_dev, b_dev, A)
    assert tk.dtype == torch.long and an.dtype == torch.float32
    assert torch.equal(tk.cpu(), torch.from_numpy(rt)) and torch.equal(an.cpu(), torch.from_numpy(ra))
    # the launcher itself, nbytes larger than needed
    nbytes = nb + 3
    wide = np.full((B, nbytes), 0xFF, np.uint8)
    wide[:, :nb] = bits
    w_dev = torch.from_numpy(wide).to(cuda())
    guard, sent_f, sent_i = 64, 0x7FC0DEAD, -0x0123456789ABCDEF
    an2 = torch.empty(B * A + guard, dtype=torch.float32, device=cuda())
    an2.view(torch.int32).fill_(sent_f)
    tk2 = torch.full((B * L + guard,), sent_i, dtype=torch.long, device=cuda())
    _lib.call("pbx_unpack_batch", t_dev.data_ptr(), w_dev.data_ptr(), tk2.data_ptr(), an2.data_ptr(), B, L, A,
              nbytes, _lib.stream_ptr(cuda()))
    torch.cuda.synchronize()
    assert torch.equal(tk2[:B * L].cpu().view(B, L), torch.from_numpy(rt))
    assert torch.equal(an2[:B * A].cpu().view(B, A), torch.from_numpy(ra))
    assert bool(torch.all(an2[B * A:].view(torch.int32) == sent_f)) and bool(torch.all(tk2[B * L:] == sent_i))
