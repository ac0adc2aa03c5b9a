"""GPU: ``pbx_token_head_loss`` / ``pbx_token_head_loss_fold`` (csrc/finetune.hip) and
``ops.finetune_head.TokenHeadLossFn`` alone: the class-weighted, label-smoothed cross-entropy of a per-residue head
over 1..8 bf16 row sources and its gradient with respect to the logits, which are never written.

Cases and inputs are those of tests/test_hip_task_calls.py (M = 111, 259, 650, 900; 900 has L = 100, so gterm's
sample index changes inside a workgroup), labels those of tests/test_hip_task_eval.py (a third -100, sequence 0 all
-100, sequence 1 all live, and a copy with ``y = K`` and ``y = 10**6`` planted).  Every case runs with ``cw`` null
and with random weights in [0.2, 1.2], and with ``eps`` 0 and 0.1.  With ``p = softmax(z)``, ``w = cw`` (or ones),
``S = sum_k w_k`` the fp64 reference of a live row is

    loss_row = (1 - eps) w_y (-log p_y) + (eps / K) sum_k w_k (-log p_k)
    g[k]     = (1 - eps) w_y (p_k - [k == y]) + (eps / K) (p_k S - w_k)

``g``: per element within ``16 * e_G + 2^-24 (|g_ref| + w_max)``, ``e_G`` the worst absolute error of an independent
fp32 torch evaluation (autograd of ``F.cross_entropy(..., reduction="sum")`` on fp32 logits), 16 the width this
project grants ``__expf`` and the FMA order.  Loss partials: the budget of tests/test_hip_task_eval.py
(``_loss_check``) with ``ce`` replaced by ``loss_row`` and ``e_L`` by the worst per-row error of the fp32 torch
``reduction="none"`` evaluation.  Weight partials: exactly the live count for ``cw`` null, otherwise within the fp32
summation error ``n 2^-24 sum w``.  Counters: exact.  Every launch twice, bitwise equal.

``TokenHeadLossFn``: loss, ``dW``, ``db``, ``dgt`` and ``dh`` against fp64 autograd of the torch definition on the
CPU, each within ``16 e + 2^-24 |ref|`` with ``e`` the worst absolute error of the same autograd in fp32 torch (the
second term is the rounding of an fp32 result); ``dh`` is returned in bf16 (8 significant bits: half an ulp is up
to ``2^-8`` of the value)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_task_calls import CASES, CH
from test_hip_task_calls import _launch as _launch_calls
from test_hip_task_eval import _ecase, _fold_loss

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -24
SENT_F, SENT_I = -7.0, -77
PAD = 64
VARIANTS = [(False, 0.0), (False, 0.1), (True, 0.0), (True, 0.1)]      # (class weights, label smoothing)


def _lib():
    from proteinbert_pytorch_replication_amd.ops import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nwg(M):
    return (M + 255) // 256


def _rows64(Z, y, w, eps):
    """fp64 ``(loss_row [M], wrow [M], g [M, K])`` by the formulas of the module docstring; zero off the live rows."""
    K = Z.shape[1]
    live = (y >= 0) & (y < K)
    ys = torch.where(live, y, torch.zeros_like(y))
    lp = torch.log_softmax(Z, -1)
    p = lp.exp()
    wy = w[ys] * live
    onehot = F.one_hot(ys, K).to(F64)
    rows = (1 - eps) * wy * -(lp.gather(-1, ys[:, None])[:, 0]) + (eps / K) * live * (w * -lp).sum(-1)
    g = (1 - eps) * wy[:, None] * (p - onehot) + (eps / K) * live[:, None] * (p * w.sum() - w)
    return rows, wy, g


@functools.lru_cache(maxsize=None)
def _lcase(B, L, nb, K, with_g):
    """The evaluation test's case plus, per variant and label set, the fp64 rows and the errors ``e_G`` / ``e_L`` of
    the independent fp32 torch evaluation: computed once and only read."""
    c = dict(_ecase(B, L, nb, K, with_g))
    M = c["M"]
    cat = torch.cat([h.cpu() for h in c["hs"]], -1)
    Z = cat.to(F64) @ c["W"].cpu().to(F64).T + c["b"].cpu().to(F64)
    Z32 = cat.float() @ c["W"].cpu().T + c["b"].cpu()
    if with_g:
        Z = Z + c["gt"].cpu().to(F64).unsqueeze(1)
        Z32 = Z32 + c["gt"].cpu().unsqueeze(1)
    Z, Z32 = Z.view(M, K), Z32.view(M, K)
    gen = torch.Generator(device="cpu").manual_seed(191 + 7 * nb + K)
    cw = 0.2 + torch.rand(K, generator=gen)                                     # [0.2, 1.2]
    ref = {}
    for weighted, eps in VARIANTS:
        w32 = cw if weighted else None
        w = cw.to(F64) if weighted else torch.ones(K, dtype=F64)
        for name in ("y", "y_bad"):
            y = c[name].cpu().view(-1)
            rows, wy, g = _rows64(Z, y, w, eps)
            yt = torch.where((y >= 0) & (y < K), y, torch.full_like(y, -100))
            z32 = Z32.clone().requires_grad_(True)
            F.cross_entropy(z32, yt, weight=w32, ignore_index=-100, label_smoothing=eps, reduction="sum").backward()
            rows32 = F.cross_entropy(Z32, yt, weight=w32, ignore_index=-100, label_smoothing=eps, reduction="none")
            ref[(weighted, eps, name)] = dict(rows=rows, wy=wy, g=g, e_G=float((z32.grad.to(F64) - g).abs().max()),
                                              e_L=float((rows32.to(F64) - rows).abs().max()))
    c.update(cw=cw.cuda(), w_max=float(cw.max()), ref=ref)
    return c


def _launch(c, y, cw, eps, M, L, K):
    """The raw launcher on the first ``M`` rows: ``(g, part, cnt)`` flat; ``g`` is NaN where it must be written, and
    all three end in ``PAD`` sentinel elements."""
    lib = _lib()
    rows = [h.view(-1, CH) for h in c["hs"]]
    srcs = (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])
    nwg = lib.lib().pbx_token_head_loss_parts(M)
    assert nwg == _nwg(M)
    g = torch.full((M * K + PAD,), float("nan"), device="cuda")
    g[M * K:] = SENT_F
    part = torch.full((nwg * 2 + PAD,), SENT_F, device="cuda")
    cnt = torch.full((nwg * 3 + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    lib.call("pbx_token_head_loss", srcs, len(rows), c["W"].data_ptr(), c["b"].data_ptr(), lib.ptr(c["gt"]),
             y.data_ptr(), lib.ptr(cw), eps, g.data_ptr(), part.data_ptr(), cnt.data_ptr(), M, K, L,
             lib.stream_ptr(g.device))
    return g, part, cnt


def _fold(part, cnt, nwg, out, acc_cnt):
    lib = _lib()
    lib.call("pbx_token_head_loss_fold", part.data_ptr(), cnt.data_ptr(), nwg, out.data_ptr(), acc_cnt.data_ptr(),
             lib.stream_ptr(part.device))


def _cpu_counts(y, call, K, M):
    """int64 [nwg, 3] (live, hits, bad) from labels and calls on the CPU: workgroup w owns rows 256 w .. 256 w + 255."""
    nwg = _nwg(M)
    wg = torch.arange(M) // 256
    live, bad = (y >= 0) & (y < K), y >= K
    out = torch.zeros(nwg, 3, dtype=torch.int64)
    for j, sel in enumerate((live, live & (call == y), bad)):
        out[:, j].index_add_(0, wg[sel], torch.ones_like(wg[sel]))
    return out


def _check(c, r, got, y, weighted, K, M, tag):
    """One launch against the reference ``r``; returns the worst err / bound of g and of the loss partials."""
    g, part, cnt = got
    nwg = _nwg(M)
    assert (g[M * K:] == SENT_F).all() and (part[2 * nwg:] == SENT_F).all() and (cnt[3 * nwg:] == SENT_I).all(), tag
    G = g[:M * K].view(M, K)
    live = (y >= 0) & (y < K)
    assert torch.isfinite(G).all(), tag                                          # every row < M was written
    assert (G[~live] == 0).all(), tag
    bound = 16 * r["e_G"] + EPS * (r["g"].abs() + (c["w_max"] if weighted else 1.0))
    err = (G.to(F64) - r["g"]).abs()
    assert (err <= bound).all(), (tag, float((err / bound).max()))
    if K == 1:
        assert (G == 0).all(), tag
    worst = 0.0
    P = part[:2 * nwg].view(nwg, 2)
    for w in range(nwg):
        sel = live[w * 256:(w + 1) * 256]
        lr = r["rows"][w * 256:(w + 1) * 256][sel]
        wy = r["wy"][w * 256:(w + 1) * 256][sel]
        n = int(sel.sum())
        if n == 0 or K == 1:
            assert _bits(P[w, 0:1]).item() == 0, (tag, w)                         # exactly +0
        else:
            budget = float((16 * r["e_L"] + EPS * (1 + lr)).sum() + n * EPS * lr.abs().sum())
            e = abs(float(P[w, 0]) - float(lr.sum()))
            worst = max(worst, e / budget)
            assert e <= budget, (tag, w, e, budget)
        if weighted:
            assert abs(float(P[w, 1]) - float(wy.sum())) <= n * EPS * float(wy.sum()), (tag, w)
        else:
            assert float(P[w, 1]) == float(n), (tag, w)
    return float((err / bound).max()), worst


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_gradient_partials_and_counters(B, L, nb, K, with_g):
    c = _lcase(B, L, nb, K, with_g)
    M, nwg = c["M"], _nwg(c["M"])
    _, lab, _ = _launch_calls(c, M, L, K, False, tokens=False)
    call = lab.cpu()[:M].long()
    assert (call >= 0).all()
    for weighted, eps in VARIANTS:
        cw = c["cw"] if weighted else None
        for name in ("y", "y_bad"):
            tag = (weighted, eps, name)
            a = _launch(c, c[name], cw, eps, M, L, K)
            b = _launch(c, c[name], cw, eps, M, L, K)
            torch.cuda.synchronize()
            a, b = [t.cpu() for t in a], [t.cpu() for t in b]
            assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b)), tag     # bitwise repeatable
            y = c[name].cpu().view(-1)
            rg, rl = _check(c, c["ref"][tag], a, y, weighted, K, M, tag)
            want = _cpu_counts(y, call, K, M)
            assert torch.equal(a[2][:3 * nwg].view(nwg, 3).long(), want), tag
            assert int(want[:, 2].sum()) == (4 if name == "y_bad" else 0), tag
            print(f"task loss B={B} L={L} nb={nb} K={K} gterm={with_g} cw={weighted} eps={eps} {name}: "
                  f"e_G {c['ref'][tag]['e_G']:.3e} e_L {c['ref'][tag]['e_L']:.3e} worst g err / bound {rg:.4f} "
                  f"loss err / budget {rl:.4f}")
    # planted labels contribute nothing: their rows are zero and the other rows are bit for bit the same
    ga, gb = (_launch(c, c[n], c["cw"], 0.1, M, L, K)[0].cpu()[:M * K].view(M, K) for n in ("y", "y_bad"))
    same = (c["y"].cpu().view(-1) == c["y_bad"].cpu().view(-1))
    assert torch.equal(_bits(ga[same]), _bits(gb[same])) and (gb[~same] == 0).all() and int((~same).sum()) == 4


@pytest.mark.parametrize("B,L,nb,K,with_g", [c for c in CASES if c[0] * c[1] >= 257])
def test_full_workgroups_are_independent_of_the_launch_size(B, L, nb, K, with_g):
    c = _lcase(B, L, nb, K, with_g)
    M = c["M"]
    g, part, cnt = (t.cpu() for t in _launch(c, c["y"], c["cw"], 0.1, M, L, K))
    for M1 in (256, 257, M - 1):
        g1, p1, c1 = (t.cpu() for t in _launch(c, c["y"], c["cw"], 0.1, M1, L, K))
        full, n1 = M1 // 256, _nwg(M1)
        assert torch.equal(_bits(g1[:M1 * K]), _bits(g[:M1 * K])), M1           # a row's gradient is its own
        assert torch.equal(_bits(p1[:2 * full]), _bits(part[:2 * full])) and torch.equal(c1[:3 * full], cnt[:3 * full])
        assert (g1[M1 * K:] == SENT_F).all() and (p1[2 * n1:] == SENT_F).all() and (c1[3 * n1:] == SENT_I).all(), M1


@pytest.mark.parametrize("B,L,nb,K,with_g", [CASES[1], CASES[8], CASES[11]])
def test_fold_of_a_batch(B, L, nb, K, with_g):
    c = _lcase(B, L, nb, K, with_g)
    M, nwg = c["M"], _nwg(c["M"])
    r = c["ref"][(True, 0.1, "y_bad")]
    _, part, cnt = _launch(c, c["y_bad"], c["cw"], 0.1, M, L, K)
    outs = [torch.full((3 + PAD,), SENT_F, device="cuda") for _ in range(2)]
    acc = torch.zeros(3 + PAD, dtype=torch.int64, device="cuda")
    for out in outs:
        _fold(part, cnt, nwg, out, acc)
    torch.cuda.synchronize()
    P = part.cpu()[:2 * nwg].view(nwg, 2)
    C = cnt.cpu()[:3 * nwg].view(nwg, 3).long().sum(0)
    sl, sw = _fold_loss(P[:, 0].tolist()), _fold_loss(P[:, 1].tolist())
    want = torch.tensor([sl / sw, 1.0 / sw, int(C[1]) / max(1, int(C[0]))], dtype=F64).float()
    for out in outs:
        out = out.cpu()
        assert torch.equal(_bits(out[:3]), _bits(want)) and (out[3:] == SENT_F).all()
    assert acc.cpu()[:3].tolist() == (2 * C).tolist() and not acc.cpu()[3:].any() and int(C[2]) == 4
    # against fp64: the partials' budgets, then the fp32 rounding of the quotient
    live = r["wy"] > 0                                                          # the weights are >= 0.2
    lr = r["rows"][live]
    n = int(live.sum())
    budget = 0.0                                                                # the workgroups' budgets, summed
    for w in range(nwg):
        sel = live[w * 256:(w + 1) * 256]
        lw = r["rows"][w * 256:(w + 1) * 256][sel]
        budget += float((16 * r["e_L"] + EPS * (1 + lw)).sum() + int(sel.sum()) * EPS * lw.abs().sum())
    ref_w = float(r["wy"].sum())
    ref = float(lr.sum()) / ref_w
    got = outs[0].cpu()
    rel_w = n * EPS
    assert abs(float(got[0]) - ref) <= budget / ref_w + (rel_w + EPS) * ref
    assert abs(float(got[1]) - 1 / ref_w) <= (rel_w + EPS) / ref_w


def test_an_all_ignored_batch_folds_to_nan_and_zero():
    B, L, nb, K, with_g = CASES[5]
    c = _lcase(B, L, nb, K, with_g)
    M, nwg = c["M"], _nwg(c["M"])
    y = torch.full((B, L), -100, dtype=torch.int64, device="cuda")
    g, part, cnt = _launch(c, y, c["cw"], 0.1, M, L, K)
    out = torch.full((3,), SENT_F, device="cuda")
    acc = torch.zeros(3, dtype=torch.int64, device="cuda")
    _fold(part, cnt, nwg, out, acc)
    out, g = out.cpu(), g.cpu()
    assert math.isnan(float(out[0])) and _bits(out[1:]).tolist() == [0, 0] and not acc.any()
    assert (_bits(g[:M * K]) == 0).all() and (_bits(part.cpu()[:2 * nwg]) == 0).all() and not cnt.cpu()[:3 * nwg].any()


@pytest.mark.parametrize("nwg", [1, 255, 257, 1000, 4100])
def test_fold_alone_at_many_workgroups(nwg):
    """Synthetic partials: runs of one and of many partials per thread.  The fp64 sums take the order of
    ``_fold_loss``; the counters are exact; two folds accumulate."""
    gen = torch.Generator(device="cpu").manual_seed(nwg)
    part = (torch.rand(nwg, 2, generator=gen) * 300).cuda()
    cnt = torch.randint(0, 257, (nwg, 3), generator=gen, dtype=torch.int32).cuda()
    out = torch.full((3 + PAD,), SENT_F, device="cuda")
    acc = torch.tensor([5, 6, 7], dtype=torch.int64, device="cuda")
    _fold(part, cnt, nwg, out, acc)
    _fold(part, cnt, nwg, out, acc)
    out = out.cpu()
    P, C = part.cpu(), cnt.cpu().long().sum(0)
    sl, sw = _fold_loss(P[:, 0].tolist()), _fold_loss(P[:, 1].tolist())
    want = torch.tensor([sl / sw, 1.0 / sw, int(C[1]) / max(1, int(C[0]))], dtype=F64).float()
    assert torch.equal(_bits(out[:3]), _bits(want)) and (out[3:] == SENT_F).all()
    assert acc.cpu().tolist() == (2 * C + torch.tensor([5, 6, 7])).tolist()


def test_invalid_arguments_raise_before_any_launch():
    lib = _lib()
    B, L, K = 3, 37, 3
    M = B * L
    h = torch.zeros(B, L, CH, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    W, b = torch.zeros(K, 9 * CH, device="cuda"), torch.zeros(17, device="cuda")
    g = torch.full((M * 17 + PAD,), SENT_F, device="cuda")
    part = torch.full((2 + PAD,), SENT_F, device="cuda")
    cnt = torch.full((3 + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    out = torch.full((3,), SENT_F, device="cuda")
    acc = torch.zeros(3, dtype=torch.int64, device="cuda")
    flat = torch.zeros((M * CH + 4,), dtype=torch.bfloat16, device="cuda")
    src = lambda *p: (ctypes.c_void_p * len(p))(*p)                 # noqa: E731
    ok = dict(srcs=src(h.data_ptr()), nb=1, W=W.data_ptr(), b=b.data_ptr(), y=y.data_ptr(), eps=0.1, g=g.data_ptr(),
              part=part.data_ptr(), cnt=cnt.data_ptr(), M=M, K=K, L=L)
    bad = [dict(eps=1.0), dict(eps=-0.01), dict(eps=float("nan")), dict(y=None),
           dict(srcs=src(*[h.data_ptr()] * 9), nb=9), dict(K=17), dict(K=0), dict(nb=0), dict(g=None),
           dict(part=None), dict(cnt=None), dict(W=None), dict(b=None), dict(srcs=None), dict(srcs=src(flat[4:].data_ptr())), dict(M=0), dict(M=-5), dict(L=0)]
    st = lib.stream_ptr(h.device)
    for kw in bad:
        a = dict(ok, **kw)
        with pytest.raises(lib.HipError, match="hipError 1$"):
            lib.call("pbx_token_head_loss", a["srcs"], a["nb"], a["W"], a["b"], None, a["y"], None, a["eps"], a["g"],
                     a["part"], a["cnt"], a["M"], a["K"], a["L"], st)
    fold_ok = dict(part=part.data_ptr(), cnt=cnt.data_ptr(), nwg=1, out=out.data_ptr(), acc=acc.data_ptr())
    for kw in (dict(part=None), dict(cnt=None), dict(out=None), dict(acc=None), dict(nwg=0)):
        a = dict(fold_ok, **kw)
        with pytest.raises(lib.HipError, match="hipError 1$"):
            lib.call("pbx_token_head_loss_fold", a["part"], a["cnt"], a["nwg"], a["out"], a["acc"], st)
    torch.cuda.synchronize()
    assert (g == SENT_F).all() and (part == SENT_F).all() and (cnt == SENT_I).all() and (out == SENT_F).all()
    assert not acc.any()
    assert lib.lib().pbx_token_head_loss_parts(0) == 0 and lib.lib().pbx_token_head_loss_parts(257) == 2
    # the autograd wrapper validates before its first launch
    from proteinbert_pytorch_replication_amd.ops.finetune_head import TokenHeadLossFn
    Wp, bp = torch.zeros(K, CH, device="cuda"), torch.zeros(K, device="cuda")
    calls = []
    real = lib.call
    lib.call = lambda *a: calls.append(a)
    try:
        for kw in (dict(eps=1.0), dict(eps=-0.5), dict(y=y.int()), dict(y=y[:, :-1]), dict(cw=torch.ones(K + 1)),
                   dict(acc=torch.zeros(3, dtype=torch.int64)), dict(W=torch.zeros(K, 2 * CH, device="cuda")),
                   dict(gt=torch.zeros(B + 1, K, device="cuda"))):
            a = dict(dict(W=Wp, gt=None, y=y, cw=None, eps=0.0, acc=acc), **kw)
            with pytest.raises(ValueError):
                TokenHeadLossFn.apply(h, a["W"], bp, a["gt"], a["y"], a["cw"], a["eps"], a["acc"])
    finally:
        lib.call = real
    assert not calls


@pytest.mark.parametrize("nb,K,with_g,weighted,eps", [(1, 3, False, True, 0.1), (1, 8, True, False, 0.0),
                                                      (3, 8, True, True, 0.1), (3, 3, False, False, 0.1)])
def test_autograd_function_against_fp64(nb, K, with_g, weighted, eps):
    from proteinbert_pytorch_replication_amd.ops import finetune_head as fh
    lib = _lib()
    B, L = 5, 130
    gen = torch.Generator(device="cpu").manual_seed(100 * nb + K)
    hs = [torch.randn(B, L, CH, generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = torch.randn(K, nb * CH, generator=gen) * 0.1
    b = torch.randn(K, generator=gen)
    gt = torch.randn(B, K, generator=gen) if with_g else None
    cw = 0.2 + torch.rand(K, generator=gen) if weighted else None
    y = torch.randint(0, K, (B, L), generator=gen)
    y[torch.rand(B, L, generator=gen) < 1.0 / 3.0] = -100
    y[0] = -100

    def run(dtype, dev, fused):
        leaves = [h.to(dev) if fused else h.to(dev, dtype) for h in hs]
        leaves += [W.to(dev, dtype), b.to(dev, dtype)] + ([gt.to(dev, dtype)] if with_g else [])
        leaves = [t.clone().requires_grad_(True) for t in leaves]
        lh, (lW, lb), lg = leaves[:nb], leaves[nb:nb + 2], (leaves[nb + 2] if with_g else None)
        w = None if cw is None else cw.to(dev, dtype)
        if fused:
            acc_cnt = torch.zeros(3, dtype=torch.int64, device=dev)
            loss, acc = fh.TokenHeadLossFn.apply(*lh, lW, lb, lg, y.to(dev), w, eps, acc_cnt)
            assert not acc.requires_grad and loss.shape == () and acc.shape == ()
        else:
            # the definition, in the leaves' precision (token_head_loss_torch is this in fp32: checked below)
            z = F.linear(torch.cat(lh, dim=-1), lW, lb)
            z = (z if lg is None else z + lg.unsqueeze(1)).reshape(-1, K)
            loss = F.cross_entropy(z, y.view(-1), weight=w, ignore_index=-100, label_smoothing=eps)
            acc, acc_cnt = torch.zeros(()), None
            if dtype == torch.float32:
                lt, at = fh.token_head_loss_torch(lh, lW, lb, lg, y, w, eps)
                hit = (z.detach().argmax(-1) == y.view(-1)).sum() / (y >= 0).sum()
                assert torch.equal(lt, loss) and abs(float(at) - float(hit)) <= 1e-6
        loss.backward()
        return loss.detach().cpu(), acc.cpu(), [t.grad.detach().cpu() for t in leaves], acc_cnt

    l64, _, g64, _ = run(F64, "cpu", False)
    l32, _, g32, _ = run(torch.float32, "cpu", False)
    calls = []
    real = lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        lk, acck, gk, cnt = run(torch.float32, "cuda", True)
        lk2, _, gk2, _ = run(torch.float32, "cuda", True)
    finally:
        lib.call = real
    half = len(calls) // 2
    assert calls[:half] == ["pbx_token_head_loss", "pbx_token_head_loss_fold",
                            "pbx_token_head_wgrad" if nb == 1 else "pbx_token_head_multi_wgrad", "pbx_colsum_add"]
    assert calls[half:] == calls[:half]
    assert torch.equal(_bits(lk), _bits(lk2)) and all(torch.equal(a, b_) for a, b_ in zip(gk, gk2))
    names = [f"dh{i}" for i in range(nb)] + ["dW", "db"] + (["dgt"] if with_g else [])
    e = abs(float(l32) - float(l64))
    assert abs(float(lk) - float(l64)) <= 16 * e + EPS * abs(float(l64)), ("loss", float(lk), float(l64), e)
    report = [f"loss e {e:.2e}"]
    for i, (name, k, r32, r64) in enumerate(zip(names, gk, g32, g64)):
        e = float((r32.to(F64) - r64).abs().max())
        bound = 16 * e + EPS * r64.abs()
        if i < nb:
            assert k.dtype == torch.bfloat16
            bound = bound + 2.0 ** -8 * (r64.abs() + bound)
        err = (k.to(F64) - r64).abs()
        report.append(f"{name} e {e:.2e} worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
    # the counters and the accuracy are those of the calls kernel's labels
    live = (y >= 0).view(-1)
    cnt = cnt.cpu().tolist()
    assert cnt[0] == int(live.sum()) and cnt[2] == 0 and float(acck) == float(torch.tensor(cnt[1] / cnt[0]).float())
    print(f"TokenHeadLossFn nb={nb} K={K} gterm={with_g} cw={weighted} eps={eps}: " + "; ".join(report))
