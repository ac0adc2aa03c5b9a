"""GPU: ``pbx_token_head_calls`` (csrc/finetune.hip, ops/infer_heads.token_head_calls) alone: prediction with a
per-residue task head over 1..8 bf16 row sources, against an fp64 CPU reference from the exact bf16 rows and the
fp32 ``W``, ``b``, ``gterm``.

Shapes: M = B * L = 111 (under one 256-row workgroup), 259 (one row past a workgroup), 650 (several workgroups
and a tail) and 900 (L = 100 does not divide 256: gterm's sample index changes inside a workgroup), crossed with
nb in {1, 2, 6, 8}, K in {1, 2, 3, 8, 16}, with and without gterm (a sample: every value of every axis at least
twice).  Tokens mix ids 0..3 with residues; sequence 0 is all <pad>, sequence 1 has no masked position.

Probabilities: within ``16 * e_P * P + 2^-24`` of the reference, e_P the worst relative error of an independent
fp32 torch evaluation of the same case (the bound, and the reasoning, of tests/test_hip_infer_heads.py for
``pbx_phead_probs``: 16 is the width granted to ``__expf`` and the FMA order).  Calls: exact on the kernel's own
stored probabilities, lowest index first.  Every launch twice, bitwise equal."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CH = 128
F64 = torch.float64
EPS = 2.0 ** -24
SENT_F, SENT_I = -7.0, -77
PAD = 64                                        # sentinel elements after every output
MIN_TOKEN = 3                                   # UNK_ID: ids 0..2 are <pad>, <sos>, <eos>
# (B, L, nb, K, gterm)
CASES = [(3, 37, 1, 1, False), (3, 37, 6, 8, True),
         (7, 37, 2, 2, True), (7, 37, 8, 16, False), (7, 37, 1, 8, True),
         (5, 130, 6, 3, False), (5, 130, 8, 1, True), (5, 130, 2, 16, True),
         (9, 100, 1, 3, False), (9, 100, 6, 2, False), (9, 100, 2, 8, False), (9, 100, 8, 3, True)]


def _lib():
    from proteinbert_pytorch_replication_amd.ops import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tokens(B, L, gen):
    t = torch.randint(0, 26, (B, L), device="cuda", generator=gen)             # ids 0, 1, 2, 3 and residues
    t[:, 0] = 1                                                                 # <sos> where a sequence starts
    t[:, L // 2] = torch.arange(B, device="cuda") % 4                           # every special id somewhere
    t[0] = 0                                                                    # an all-<pad> sequence
    t[1] = torch.randint(MIN_TOKEN, 26, (L,), device="cuda", generator=gen)     # no masked position at all
    return t


@functools.lru_cache(maxsize=None)
def _case(B, L, nb, K, with_g):
    """Seeded inputs on the GPU, the fp64 CPU reference ``P = softmax(Z, -1)`` and ``e_P`` of the independent
    fp32 evaluation: computed once per case and only read."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * nb + 10 * K + B)
    hs = [torch.randn(B, L, CH, device="cuda", generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = torch.randn(K, nb * CH, device="cuda", generator=gen) * 0.1
    b = torch.randn(K, device="cuda", generator=gen)
    gt = torch.randn(B, K, device="cuda", generator=gen) if with_g else None
    tokens = _tokens(B, L, gen)
    cat = torch.cat([h.cpu() for h in hs], -1)                                  # [B, L, nb*128] bf16, exact
    Z = cat.to(F64) @ W.cpu().to(F64).T + b.cpu().to(F64)
    Z32 = cat.float() @ W.cpu().T + b.cpu()
    if with_g:
        Z = Z + gt.cpu().to(F64).unsqueeze(1)
        Z32 = Z32 + gt.cpu().unsqueeze(1)
    P = torch.softmax(Z, -1)
    e_P = float(((torch.softmax(Z32, -1).to(F64) - P).abs() / P).max())
    live = (tokens >= MIN_TOKEN).cpu()
    assert not live[0].any() and live[1].all() and live.any() and (~live[2:]).any()
    return dict(hs=hs, W=W, b=b, gt=gt, tokens=tokens, P=P, e_P=e_P, live=live, M=B * L)


def _launch(c, M, L, K, store, tokens=True):
    """The raw launcher on the first ``M`` rows, into sentinel-padded buffers: ``(probs | None, labels, pmax)``
    as flat tensors with ``PAD`` sentinel elements after the outputs."""
    lib = _lib()
    rows = [h.view(-1, CH) for h in c["hs"]]
    srcs = (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])
    probs = torch.full((M * K + PAD,), SENT_F, device="cuda") if store else None
    labels = torch.full((M + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    pmax = torch.full((M + PAD,), SENT_F, device="cuda")
    lib.call("pbx_token_head_calls", srcs, len(rows), c["W"].data_ptr(), c["b"].data_ptr(), lib.ptr(c["gt"]),
             c["tokens"].data_ptr() if tokens else None, MIN_TOKEN, lib.ptr(probs), labels.data_ptr(), pmax.data_ptr(),
             M, K, L, lib.stream_ptr(labels.device))
    return probs, labels, pmax


@functools.lru_cache(maxsize=None)
def _full(B, L, nb, K, with_g):
    """The full launch of a case with the probability store, on the CPU (shared by the tests below)."""
    c = _case(B, L, nb, K, with_g)
    res = _launch(c, c["M"], L, K, True)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in res)


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_probabilities_calls_masks_and_bounds(B, L, nb, K, with_g):
    c = _case(B, L, nb, K, with_g)
    M, live = c["M"], c["live"].view(-1)
    probs, labels, pmax = _full(B, L, nb, K, with_g)
    again = _launch(c, M, L, K, True)
    _, labels_n, pmax_n = _launch(c, M, L, K, False)
    torch.cuda.synchronize()
    # bitwise repeatable; nothing written past the outputs
    assert all(torch.equal(_bits(a), _bits(b.cpu())) for a, b in zip((probs, labels, pmax), again))
    assert (probs[M * K:] == SENT_F).all() and (labels[M:] == SENT_I).all() and (pmax[M:] == SENT_F).all()
    assert (labels_n.cpu()[M:] == SENT_I).all() and (pmax_n.cpu()[M:] == SENT_F).all()
    P, lab, pm = probs[:M * K].view(M, K), labels[:M].long(), pmax[:M]
    # masked rows: label -1, pmax 0, a zero row; every other row fully written
    assert (lab[~live] == -1).all() and (_bits(pm[~live]) == 0).all() and (_bits(P[~live]) == 0).all()
    assert (lab[live] >= 0).all() and not (P[live] == SENT_F).any()
    # the calls: exact on the stored probabilities (first maximal index), with or without the store
    assert torch.equal(lab[live], P[live].argmax(-1))
    assert torch.equal(_bits(pm[live]), _bits(P[live].gather(-1, lab[live].unsqueeze(-1)).squeeze(-1)))
    assert torch.equal(labels_n.cpu()[:M].long(), lab) and torch.equal(_bits(pmax_n.cpu()[:M]), _bits(pm))
    # the probabilities against fp64
    ref = c["P"].view(M, K)[live]
    err = (P[live].to(F64) - ref).abs()
    bound = 16 * c["e_P"] * ref + EPS
    print(f"task calls B={B} L={L} nb={nb} K={K} gterm={with_g}: e_P {c['e_P']:.3e} worst err / bound "
          f"{float((err / bound).max()):.3f} worst rel err {float((err / ref).max()):.3e} min P {float(ref.min()):.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("B,L,nb,K,with_g", [c for c in CASES if c[0] * c[1] >= 257])
def test_rows_are_independent_of_the_launch_size(B, L, nb, K, with_g):
    c = _case(B, L, nb, K, with_g)
    probs, labels, pmax = _full(B, L, nb, K, with_g)
    for M1 in (255, 256, 257):
        p1, l1, m1 = (t.cpu() for t in _launch(c, M1, L, K, True))
        assert torch.equal(_bits(p1[:M1 * K]), _bits(probs[:M1 * K])), M1
        assert torch.equal(l1[:M1], labels[:M1]) and torch.equal(_bits(m1[:M1]), _bits(pmax[:M1])), M1
        assert (p1[M1 * K:] == SENT_F).all() and (l1[M1:] == SENT_I).all() and (m1[M1:] == SENT_F).all(), M1


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_wrapper_matches_the_launcher_and_the_torch_form(B, L, nb, K, with_g):
    from proteinbert_pytorch_replication_amd.ops import infer_heads as ih
    c = _case(B, L, nb, K, with_g)
    probs, labels, pmax = _full(B, L, nb, K, with_g)
    M = c["M"]
    buf = torch.full((M * K + PAD,), SENT_F, device="cuda")
    P, lab, pm = ih.token_head_calls(c["hs"], c["W"], c["b"], c["gt"], c["tokens"], store_probs=True,
                                     out=buf[:M * K].view(B, L, K))
    Pn, lab_n, pm_n = ih.token_head_calls(c["hs"], c["W"], c["b"], c["gt"], c["tokens"])
    # a misaligned source (8 bytes off a 16-byte boundary) is cloned by the wrapper, not read in place
    flat = torch.empty((M * CH + 4,), dtype=torch.bfloat16, device="cuda")
    off = flat[4:].view(B, L, CH)
    off.copy_(c["hs"][0])
    assert off.data_ptr() % 16 != 0
    _, lab_o, pm_o = ih.token_head_calls([off] + c["hs"][1:], c["W"], c["b"], c["gt"], c["tokens"])
    torch.cuda.synchronize()
    assert P.data_ptr() == buf.data_ptr() and Pn is None and (buf[M * K:] == SENT_F).all()
    assert P.shape == (B, L, K) and lab.shape == pm.shape == (B, L)
    assert lab.dtype == torch.int32 and pm.dtype == P.dtype == torch.float32
    assert torch.equal(_bits(P.cpu().view(-1)), _bits(probs[:M * K]))
    for l_, m_ in ((lab, pm), (lab_n, pm_n), (lab_o, pm_o)):
        assert torch.equal(l_.cpu().view(-1), labels[:M]) and torch.equal(_bits(m_.cpu().view(-1)), _bits(pmax[:M]))
    # without tokens every row is live, and the live rows are the ones computed above
    _, lab_all, pm_all = ih.token_head_calls(c["hs"], c["W"], c["b"], c["gt"])
    live = c["live"]
    assert (lab_all.cpu() >= 0).all() and torch.equal(lab_all.cpu()[live], lab.cpu()[live])
    assert torch.equal(_bits(pm_all.cpu()[live]), _bits(pm.cpu()[live]))
    # the definition in torch on the same device: the same masks, probabilities within the bound
    Pt, lab_t, pm_t = ih.token_head_calls_torch(c["hs"], c["W"], c["b"], c["gt"], c["tokens"], store_probs=True)
    assert torch.equal(lab_t.cpu() < 0, ~live) and (Pt.cpu()[~live] == 0).all() and (pm_t.cpu()[~live] == 0).all()
    assert ((Pt.cpu().to(F64) - c["P"]).abs()[live] <= 16 * c["e_P"] * c["P"][live] + EPS).all()


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_consistent_with_the_training_forward(B, L, nb, K, with_g):
    """fp32 torch softmax of the logits the training kernels store lies within the bound of the kernel's
    probabilities (the kernel forms the same logits in registers)."""
    lib = _lib()
    c = _case(B, L, nb, K, with_g)
    M, live = c["M"], c["live"].view(-1)
    probs = _full(B, L, nb, K, with_g)[0][:M * K].view(M, K)
    rows = [h.view(M, CH) for h in c["hs"]]
    srcs = (ctypes.c_void_p * nb)(*[r.data_ptr() for r in rows])
    forms = {"multi_fwd": torch.empty((M, K), device="cuda")}
    lib.call("pbx_token_head_multi_fwd", srcs, nb, c["W"].data_ptr(), c["b"].data_ptr(), lib.ptr(c["gt"]),
             forms["multi_fwd"].data_ptr(), M, K, L, lib.stream_ptr(rows[0].device))
    if nb == 1 and not with_g:
        forms["fwd"] = torch.empty((M, K), device="cuda")
        lib.call("pbx_token_head_fwd", rows[0].data_ptr(), c["W"].data_ptr(), c["b"].data_ptr(),
                 forms["fwd"].data_ptr(), M, K, lib.stream_ptr(rows[0].device))
    ref = c["P"].view(M, K)[live]
    for name, Z in forms.items():
        soft = torch.softmax(Z, -1).cpu()[live]
        err = (soft.to(F64) - probs[live].to(F64)).abs()
        bound = 16 * c["e_P"] * ref + EPS
        print(f"task calls vs softmax({name}) B={B} L={L} nb={nb} K={K}: worst err / bound "
              f"{float((err / bound).max()):.3f}")
        assert (err <= bound).all(), name


def _tie_inputs(device):
    gen = torch.Generator(device="cpu").manual_seed(7)
    B, L = 7, 37
    hs = [torch.randn(B, L, CH, generator=gen).to(torch.bfloat16).to(device) for _ in range(2)]
    W = torch.randn(3, 2 * CH, generator=gen) * 0.1
    W[2] = W[1]                                                                 # classes 1 and 2: identical rows
    b = torch.tensor([0.25, -0.5, -0.5])
    gt = torch.randn(B, 3, generator=gen)
    gt[:, 2] = gt[:, 1]
    return hs, W.to(device), b.to(device), gt.to(device)


def _check_ties(fn, device):
    B, L = 7, 37
    hs, _, _, _ = _tie_inputs(device)
    # W = 0: the logits are b itself; classes 1 and 2 tie for the maximum and the lower one is called
    W0, b0 = torch.zeros(4, 2 * CH, device=device), torch.tensor([0.0, 1.0, 1.0, 0.5], device=device)
    P, lab, pm = fn(hs, W0, b0, store_probs=True)
    assert (lab == 1).all() and torch.equal(P[..., 1], P[..., 2]) and torch.equal(pm, P[..., 1])
    assert (P == P[0, 0]).all()
    # two identical classes: their probabilities are equal in every row, and the pair is called as its lower index
    hs, W, b, gt = _tie_inputs(device)
    P, lab, pm = fn(hs, W, b, gt, store_probs=True)
    same = _bits(P[..., 1]) == _bits(P[..., 2])
    if device == "cuda":                            # one thread, the same FMA sequence on the same numbers
        assert same.all()
    pair = same & (P[..., 1] > P[..., 0])
    assert pair.any() and (same & ~pair).any()
    assert (lab[pair] == 1).all() and (lab[same & ~pair] == 0).all() and not (lab[same] == 2).any()
    assert torch.equal(_bits(pm[same]), _bits(torch.where(pair, P[..., 1], P[..., 0])[same]))


def test_ties_call_the_lowest_class():
    from proteinbert_pytorch_replication_amd.ops import infer_heads as ih
    _check_ties(ih.token_head_calls_torch, "cpu")       # the construction holds by definition, on the CPU first
    _check_ties(ih.token_head_calls, "cuda")
    torch.cuda.synchronize()


def test_invalid_arguments_raise_before_any_launch():
    from proteinbert_pytorch_replication_amd.ops import infer_heads as ih
    lib = _lib()
    B, L = 3, 37
    h = torch.zeros(B, L, CH, dtype=torch.bfloat16, device="cuda")
    w = lambda K, nb=1: torch.zeros(K, nb * CH, device="cuda")      # noqa: E731
    bias = lambda K: torch.zeros(K, device="cuda")                  # noqa: E731
    bad = [dict(hs=[h], weight=w(0), bias=bias(0)),                                             # K = 0
           dict(hs=[h], weight=w(17), bias=bias(17)),                                           # K = 17
           dict(hs=[h] * 9, weight=w(3, 9), bias=bias(3)),                                      # nb = 9
           dict(hs=[h], weight=w(3), bias=bias(3), gterm=torch.zeros(B + 1, 3, device="cuda")),
           dict(hs=[h], weight=w(3), bias=bias(3), gterm=torch.zeros(B, 4, device="cuda")),
           dict(hs=[h], weight=w(3), bias=bias(3), store_probs=True, out=torch.zeros(B, L, 4, device="cuda")),
           dict(hs=[h], weight=w(3), bias=bias(3), store_probs=True, out=torch.zeros(B * L, 3, device="cuda")),
           dict(hs=[h], weight=w(3, 2), bias=bias(3)),                                          # W for two sources
           dict(hs=[h], weight=w(3), bias=bias(3), tokens=torch.zeros(B, L, dtype=torch.int32, device="cuda")),
           dict(hs=[h.float()], weight=w(3), bias=bias(3))]                                     # not bf16
    calls = []
    real = lib.call
    lib.call = lambda *a: calls.append(a)           # any launch attempt would be recorded
    try:
        for kw in bad:
            with pytest.raises(ValueError):
                ih.token_head_calls(**kw)
    finally:
        lib.call = real
    assert not calls
