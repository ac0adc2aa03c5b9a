"""GPU: ``pbx_token_head_eval`` / ``pbx_task_eval_fold`` (csrc/finetune.hip, ops/task_eval.py) alone: the
cross-entropy partials and the K x K confusion table of a per-residue head over 1..8 bf16 row sources.

Cases and inputs are those of tests/test_hip_task_calls.py (M = 111, 259, 650, 900; 900 has L = 100, so gterm's
sample index changes inside a workgroup).  Labels: uniform in 0..K-1, about a third -100; sequence 0 is all -100,
sequence 1 has none.

Counts: exact integer equality with the matrix built on the CPU from the labels ``pbx_token_head_calls`` returns
on the same inputs (the two kernels hold identical logits), per workgroup, summed, and folded.  Against the fp64
reference calls a row may disagree only where the reference's top two probabilities differ by at most twice the
probability bound of tests/test_hip_task_calls.py (``16 * e_P * P + 2^-24``); such rows are at most 1 % of the
live rows.

Loss partials: every workgroup's partial against the fp64 sum of ``ce_ref`` over its live rows, within
``sum_rows (16 * e_L + 2^-24 (1 + ce_ref)) + n 2^-24 sum |ce_ref|``: ``e_L`` is the worst absolute per-row error
of an independent fp32 torch evaluation of the case, 16 the width this project grants ``__expf`` and the FMA order,
``2^-24 (1 + ce_ref)`` the rounding of ``logf`` and the final subtraction, the last term the fp32 summation of n
rows.  For K = 1 the kernel's loss is exactly 0.  Every launch twice, bitwise equal."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_hip_task_calls import CASES, CH, _case, _tie_inputs
from test_hip_task_calls import _launch as _launch_calls

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -24
SENT_F, SENT_I = -7.0, -77
PAD = 64                                        # sentinel elements after both partial buffers


def _lib():
    from proteinbert_pytorch_replication_amd.ops import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nwg(M):
    return (M + 255) // 256


@functools.lru_cache(maxsize=None)
def _ecase(B, L, nb, K, with_g):
    """The calls test's inputs plus labels, the fp64 per-row cross-entropy, ``e_L`` and the reference calls:
    computed once per case and only read."""
    c = dict(_case(B, L, nb, K, with_g))
    gen = torch.Generator(device="cpu").manual_seed(77 + 1000 * nb + 10 * K + B)
    y = torch.randint(0, K, (B, L), generator=gen)
    y[torch.rand(B, L, generator=gen) < 1.0 / 3.0] = -100
    y[0] = -100                                                                 # a sequence that is ignored
    y[1] = torch.randint(0, K, (L,), generator=gen)                             # and one with every position live
    M = B * L
    cat = torch.cat([h.cpu() for h in c["hs"]], -1)                             # [B, L, nb*128] bf16, exact
    Z = cat.to(F64) @ c["W"].cpu().to(F64).T + c["b"].cpu().to(F64)
    Z32 = cat.float() @ c["W"].cpu().T + c["b"].cpu()
    if with_g:
        Z = Z + c["gt"].cpu().to(F64).unsqueeze(1)
        Z32 = Z32 + c["gt"].cpu().unsqueeze(1)
    Z, Z32, yf = Z.view(M, K), Z32.view(M, K), y.view(-1)
    live = yf >= 0
    ys = yf.clamp_min(0)
    ce = torch.logsumexp(Z, -1) - Z.gather(-1, ys.unsqueeze(-1)).squeeze(-1)    # fp64, every row (as if y = ys)
    ce32 = F.cross_entropy(Z32, ys, reduction="none")
    e_L = float((ce32.to(F64) - ce).abs()[live].max())
    P = c["P"].view(M, K)
    top = P.sort(-1, descending=True).values
    near = torch.zeros(M, dtype=torch.bool) if K == 1 else \
        (top[:, 0] - top[:, 1]) <= 2 * (16 * c["e_P"] * top[:, 0] + EPS)
    # planted bad labels: y = K and y = 10**6 on rows that were live, in different workgroups where there are several
    y_bad = yf.clone()
    rows = live.nonzero().view(-1)
    planted = rows[[0, len(rows) // 2, len(rows) - 1, len(rows) // 3]]
    y_bad[planted[:2]] = K
    y_bad[planted[2:]] = 10 ** 6
    assert live.view(B, L)[1].all() and not live.view(B, L)[0].any() and len(set(planted.tolist())) == 4
    c.update(y=y.cuda(), y_bad=y_bad.view(B, L).cuda(), ce=ce, e_L=e_L, ref_call=P.argmax(-1), near=near)
    return c


def _launch(c, y, M, L, K):
    """The raw launcher on the first ``M`` rows into sentinel-padded buffers: ``(loss_part, cnt_part)`` flat."""
    lib = _lib()
    rows = [h.view(-1, CH) for h in c["hs"]]
    srcs = (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])
    nwg = lib.lib().pbx_token_head_eval_parts(M)
    assert nwg == _nwg(M)
    lp = torch.full((nwg + PAD,), SENT_F, device="cuda")
    cp = torch.full((nwg * (K * K + 2) + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    lib.call("pbx_token_head_eval", srcs, len(rows), c["W"].data_ptr(), c["b"].data_ptr(), lib.ptr(c["gt"]),
             y.data_ptr(), lp.data_ptr(), cp.data_ptr(), M, K, L, lib.stream_ptr(lp.device))
    return lp, cp


def _fold(lp, cp, nwg, K, nseq, acc):
    lib = _lib()
    lib.call("pbx_task_eval_fold", lp.data_ptr(), cp.data_ptr(), nwg, K, nseq, acc.loss.data_ptr(),
             acc.counts.data_ptr(), lib.stream_ptr(lp.device))


def _cpu_tables(y, call, K, M):
    """int64 [nwg, K*K + 2] from labels and calls on the CPU: workgroup w owns rows 256 w .. 256 w + 255."""
    nwg = _nwg(M)
    out = torch.zeros(nwg, K * K + 2, dtype=torch.int64)
    wg = torch.arange(M) // 256
    live, bad = (y >= 0) & (y < K), y >= K
    idx = wg[live] * (K * K + 2) + y[live] * K + call[live]
    out.view(-1).index_add_(0, idx, torch.ones_like(idx))
    out[:, K * K] = torch.zeros(nwg, dtype=torch.int64).index_add_(0, wg[live], torch.ones_like(wg[live]))
    out[:, K * K + 1] = torch.zeros(nwg, dtype=torch.int64).index_add_(0, wg[bad], torch.ones_like(wg[bad]))
    return out


def _loss_check(c, lp, y, K, M, tag):
    """Every workgroup's loss partial against the fp64 sum over its live rows, within the budget of the module
    docstring; returns the worst err / budget."""
    live = (y >= 0) & (y < K)
    worst = 0.0
    for w in range(_nwg(M)):
        sel = live[w * 256:(w + 1) * 256]
        ce = c["ce"][w * 256:(w + 1) * 256][sel]
        n = int(sel.sum())
        budget = float((16 * c["e_L"] + EPS * (1 + ce)).sum() + n * EPS * ce.abs().sum())
        err = abs(float(lp[w]) - float(ce.sum()))
        if n == 0 or K == 1:
            assert _bits(lp[w:w + 1]).item() == 0, (tag, w)                      # exactly +0
        else:
            worst = max(worst, err / budget)
            assert err <= budget, (tag, w, err, budget)
    return worst


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_counts_exact_and_loss_partials_within_budget(B, L, nb, K, with_g):
    from proteinbert_pytorch_replication_amd.ops.task_eval import TaskEvalAccumulator
    c = _ecase(B, L, nb, K, with_g)
    M, NC, nwg = c["M"], K * K + 2, _nwg(c["M"])
    lp, cp = _launch(c, c["y"], M, L, K)
    lp2, cp2 = _launch(c, c["y"], M, L, K)
    lpb, cpb = _launch(c, c["y_bad"], M, L, K)
    _, lab, _ = _launch_calls(c, M, L, K, False, tokens=False)
    acc = TaskEvalAccumulator(K, "cuda")
    _fold(lp, cp, nwg, K, B, acc)
    torch.cuda.synchronize()
    lp, cp, lp2, cp2, lpb, cpb = (t.cpu() for t in (lp, cp, lp2, cp2, lpb, cpb))
    # bitwise repeatable; nothing written past the partials
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(cp, cp2)
    for a, b in ((lp, cp), (lpb, cpb)):
        assert (a[nwg:] == SENT_F).all() and (b[nwg * NC:] == SENT_I).all()
        assert not (a[:nwg] == SENT_F).any() and not (b[:nwg * NC] == SENT_I).any()
    # the tables: exactly those of the calls kernel's labels, per workgroup, summed and folded
    call = lab.cpu()[:M].long()
    assert (call >= 0).all()
    y = c["y"].cpu().view(-1)
    want = _cpu_tables(y, call, K, M)
    got = cp[:nwg * NC].view(nwg, NC).long()
    assert torch.equal(got, want)
    assert int(got[:, K * K].sum()) == int(((y >= 0) & (y < K)).sum()) and int(got[:, K * K + 1].sum()) == 0
    counts = acc.counts.cpu()
    assert acc.counts.dtype == torch.int64 and acc.loss.dtype == F64 and acc.confusion.shape == (K, K)
    assert torch.equal(counts[:NC], want.sum(0)) and counts[NC:].tolist() == [1, B]
    assert torch.equal(acc.confusion.cpu(), want.sum(0)[:K * K].view(K, K))
    # planted bad labels: counted in their slot, in neither the matrix nor the loss
    yb = c["y_bad"].cpu().view(-1)
    wantb = _cpu_tables(yb, call, K, M)
    gotb = cpb[:nwg * NC].view(nwg, NC).long()
    assert torch.equal(gotb, wantb) and int(gotb[:, K * K + 1].sum()) == 4
    assert int(gotb[:, K * K].sum()) == int(got[:, K * K].sum()) - 4
    assert int(gotb[:, :K * K].sum()) == int(got[:, :K * K].sum()) - 4
    # against the fp64 reference calls: disagreement only at near-ties, and those are rare
    live = y >= 0
    differ = live & (call != c["ref_call"])
    assert not (differ & ~c["near"]).any()
    share = float((live & c["near"]).sum()) / float(live.sum())
    assert share <= 0.01
    # the loss partials
    r1 = _loss_check(c, lp, y, K, M, "y")
    r2 = _loss_check(c, lpb, yb, K, M, "y_bad")
    print(f"task eval B={B} L={L} nb={nb} K={K} gterm={with_g}: e_L {c['e_L']:.3e} worst loss err / budget "
          f"{max(r1, r2):.4f} near-tie share {share:.2e} differing calls {int(differ.sum())}")


@pytest.mark.parametrize("B,L,nb,K,with_g", [c for c in CASES if c[0] * c[1] >= 257])
def test_full_workgroups_are_independent_of_the_launch_size(B, L, nb, K, with_g):
    c = _ecase(B, L, nb, K, with_g)
    M, NC = c["M"], K * K + 2
    lp, cp = (t.cpu() for t in _launch(c, c["y"], M, L, K))
    for M1 in (256, 257, M - 1):
        l1, c1 = (t.cpu() for t in _launch(c, c["y"], M1, L, K))
        full, n1 = M1 // 256, _nwg(M1)
        assert torch.equal(_bits(l1[:full]), _bits(lp[:full])), M1
        assert torch.equal(c1[:full * NC], cp[:full * NC]), M1
        assert (l1[n1:] == SENT_F).all() and (c1[n1 * NC:] == SENT_I).all(), M1
        assert int(c1[:n1 * NC].view(n1, NC)[:, K * K].sum()) == int((c["y"].view(-1)[:M1] >= 0).sum()), M1


def test_a_workgroup_without_live_rows_writes_zeros():
    B, L, nb, K, with_g = 5, 130, 6, 3, False
    c = _ecase(B, L, nb, K, with_g)
    y = c["y"].clone().view(-1)
    y[256:512] = -100                                                           # workgroup 1 of 3 sees no live row
    lp, cp = (t.cpu() for t in _launch(c, y, c["M"], L, K))
    NC = K * K + 2
    assert _bits(lp[1:2]).item() == 0 and (cp[NC:2 * NC] == 0).all()
    assert lp[0] > 0 and lp[2] > 0 and (lp[3:] == SENT_F).all()


def _fold_loss(parts):
    """The fold kernel's fp64 sum of one batch's loss partials (python floats are fp64): ascending at every level:
    256 contiguous runs of ceil(nwg / 256) partials, the run sums in 16 groups of 16, the 16 group sums."""
    nwg = len(parts)
    run = (nwg + 255) // 256
    runs = []
    for t in range(256):
        a = 0.0
        for v in parts[min(nwg, t * run):min(nwg, (t + 1) * run)]:
            a += v
        runs.append(a)
    groups = []
    for t in range(16):
        s = runs[16 * t]
        for v in runs[16 * t + 1:16 * t + 16]:
            s += v
        groups.append(s)
    s = groups[0]
    for v in groups[1:]:
        s += v
    return s


@pytest.mark.parametrize("nwg,K", [(1, 8), (255, 1), (257, 8), (1000, 16), (4100, 8), (5000, 3)])
def test_fold_alone_at_many_workgroups(nwg, K):
    """The fold on synthetic partials: one row range (up to 256 workgroups), several, and the 16-range cap; runs
    of one and of many loss partials.  Two folds into one accumulator, twice: exact sums, bitwise repeatable."""
    from proteinbert_pytorch_replication_amd.ops.task_eval import TaskEvalAccumulator
    gen = torch.Generator(device="cpu").manual_seed(nwg + K)
    NC = K * K + 2
    lp = (torch.rand(nwg, generator=gen) * 300).cuda()
    cp = torch.randint(0, 257, (nwg, NC), generator=gen, dtype=torch.int32).cuda()
    accs = [TaskEvalAccumulator(K, "cuda") for _ in range(2)]
    for acc in accs:
        _fold(lp, cp, nwg, K, 5, acc)
        _fold(lp, cp, nwg, K, 7, acc)
    torch.cuda.synchronize()
    s = _fold_loss(lp.cpu().tolist())
    for acc in accs:
        assert acc.loss.item() == (0.0 + s) + s
        assert torch.equal(acc.counts.cpu()[:NC], 2 * cp.cpu().long().sum(0))
        assert acc.counts.cpu()[NC:].tolist() == [2, 12]


def test_fold_of_two_batches_is_the_exact_sum():
    """The accumulator after two folds: the integer sums of the partials, and the fp64 sum of the loss partials
    in ascending workgroup order (``_fold_loss``), batch by batch.  Batch and sequence counters advance by 1 and
    n_sequences."""
    from proteinbert_pytorch_replication_amd.ops.task_eval import TaskEvalAccumulator
    K = 8
    ca, cb = _ecase(7, 37, 1, 8, True), _ecase(9, 100, 2, 8, False)
    acc = TaskEvalAccumulator(K, "cuda")
    parts = []
    for c, (B, L) in ((ca, (7, 37)), (cb, (9, 100))):
        lp, cp = _launch(c, c["y_bad"], c["M"], L, K)
        _fold(lp, cp, _nwg(c["M"]), K, B, acc)
        parts.append((lp.cpu()[:_nwg(c["M"])], cp.cpu()[:_nwg(c["M"]) * (K * K + 2)].view(-1, K * K + 2).long()))
    torch.cuda.synchronize()
    loss = 0.0
    for lp, _ in parts:
        loss += _fold_loss(lp.tolist())
    assert acc.loss.cpu().item() == loss
    want = parts[0][1].sum(0) + parts[1][1].sum(0)
    assert torch.equal(acc.counts.cpu()[:K * K + 2], want) and int(want[K * K + 1]) == 8
    assert acc.counts.cpu()[K * K + 2:].tolist() == [2, 7 + 9]
    acc.zero_()
    assert not acc.counts.any() and not acc.loss.any()


def test_ties_call_the_lowest_class():
    from proteinbert_pytorch_replication_amd.ops import task_eval as te
    B, L = 7, 37
    y = (torch.arange(B * L).view(B, L) % 3)
    for dev, fn in (("cpu", te.token_head_eval_torch), ("cuda", te.token_head_eval)):
        # W = 0: the logits are b itself; classes 1 and 2 tie for the maximum and the lower one is called
        hs, _, _, _ = _tie_inputs(dev)
        W0, b0 = torch.zeros(4, 2 * CH, device=dev), torch.tensor([0.0, 1.0, 1.0, 0.5], device=dev)
        acc = te.TaskEvalAccumulator(4, dev)
        fn(hs, W0, b0, None, y.to(dev), acc)
        cm = acc.confusion.cpu()
        assert torch.equal(cm[:, 1], torch.bincount(y.view(-1), minlength=4)) and int(cm.sum()) == B * L
    # two identical classes (one thread, the same FMA sequence on the same numbers): never called as the higher one
    hs, W, b, gt = _tie_inputs("cuda")
    acc = te.TaskEvalAccumulator(3, "cuda")
    te.token_head_eval(hs, W, b, gt, y.cuda(), acc)
    cm = acc.confusion.cpu()
    assert int(cm[:, 2].sum()) == 0 and int(cm[:, 1].sum()) > 0 and int(cm[:, 0].sum()) > 0 and int(cm.sum()) == B * L


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_wrapper_matches_the_launcher_and_the_torch_form(B, L, nb, K, with_g):
    from proteinbert_pytorch_replication_amd.ops import task_eval as te
    c = _ecase(B, L, nb, K, with_g)
    M, nwg = c["M"], _nwg(c["M"])
    raw = te.TaskEvalAccumulator(K, "cuda")
    lp, cp = _launch(c, c["y"], M, L, K)
    _fold(lp, cp, nwg, K, B, raw)
    acc = te.TaskEvalAccumulator(K, "cuda")
    te.token_head_eval(c["hs"], c["W"], c["b"], c["gt"], c["y"], acc)
    # a misaligned source (8 bytes off a 16-byte boundary) is cloned by the wrapper, not read in place
    flat = torch.empty((M * CH + 4,), dtype=torch.bfloat16, device="cuda")
    off = flat[4:].view(B, L, CH)
    off.copy_(c["hs"][0])
    assert off.data_ptr() % 16 != 0
    acc_o = te.TaskEvalAccumulator(K, "cuda")
    te.token_head_eval([off] + c["hs"][1:], c["W"], c["b"], c["gt"], c["y"], acc_o)
    for a in (acc, acc_o):
        assert torch.equal(a.counts, raw.counts) and torch.equal(a.loss.view(torch.int64), raw.loss.view(torch.int64))
    # the definition in torch on the same device, the near-tie rows of the fp64 reference left out
    y = c["y"].clone()
    y.view(-1)[c["near"].cuda()] = -100
    a_k, a_t = te.TaskEvalAccumulator(K, "cuda"), te.TaskEvalAccumulator(K, "cuda")
    te.token_head_eval(c["hs"], c["W"], c["b"], c["gt"], y, a_k)
    te.token_head_eval_torch(c["hs"], c["W"], c["b"], c["gt"], y, a_t)
    assert torch.equal(a_k.counts, a_t.counts)
    live = (y.cpu().view(-1) >= 0)
    ce = c["ce"][live]
    budget = float((16 * c["e_L"] + EPS * (1 + ce)).sum() + int(live.sum()) * EPS * ce.abs().sum())
    for a in (a_k, a_t):
        assert abs(a.loss.item() - float(ce.sum())) <= budget
    m = te.metrics_from_confusion(a_k)
    assert m["n"] == int(live.sum()) and m["n_batches"] == 1 and m["n_sequences"] == B
    assert abs(m["loss"] * m["n"] - a_k.loss.item()) <= 1e-9 * max(1.0, a_k.loss.item())


def test_invalid_arguments_raise_before_any_launch():
    from proteinbert_pytorch_replication_amd.ops import task_eval as te
    lib = _lib()
    B, L, K = 3, 37, 3
    M, NC = B * L, K * K + 2
    h = torch.zeros(B, L, CH, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    W, b = torch.zeros(K, 9 * CH, device="cuda"), torch.zeros(16, device="cuda")
    lp = torch.full((1 + PAD,), SENT_F, device="cuda")
    cp = torch.full((17 * 17 + 2 + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    acc = te.TaskEvalAccumulator(K, "cuda")
    flat = torch.zeros((M * CH + 4,), dtype=torch.bfloat16, device="cuda")
    src = lambda *p: (ctypes.c_void_p * len(p))(*p)                 # noqa: E731
    ok = dict(srcs=src(h.data_ptr()), nb=1, lp=lp.data_ptr(), cp=cp.data_ptr(), M=M, K=K, L=L)
    bad = [dict(lp=None), dict(cp=None), dict(K=0), dict(K=17), dict(nb=0), dict(srcs=src(*[h.data_ptr()] * 9), nb=9),
           dict(srcs=src(flat[4:].data_ptr())), dict(srcs=None), dict(M=0), dict(M=-5), dict(L=0)]
    st = lib.stream_ptr(h.device)
    for kw in bad:
        a = dict(ok, **kw)
        with pytest.raises(lib.HipError, match="hipError 1$"):
            lib.call("pbx_token_head_eval", a["srcs"], a["nb"], W.data_ptr(), b.data_ptr(), None, y.data_ptr(),
                     a["lp"], a["cp"], a["M"], a["K"], a["L"], st)
    fold_ok = dict(lp=lp.data_ptr(), cp=cp.data_ptr(), nwg=1, K=K, loss=acc.loss.data_ptr(), cnt=acc.counts.data_ptr())
    for kw in (dict(lp=None), dict(cp=None), dict(loss=None), dict(cnt=None), dict(K=0), dict(K=17), dict(nwg=0)):
        a = dict(fold_ok, **kw)
        with pytest.raises(lib.HipError, match="hipError 1$"):
            lib.call("pbx_task_eval_fold", a["lp"], a["cp"], a["nwg"], a["K"], B, a["loss"], a["cnt"], st)
    torch.cuda.synchronize()
    assert (lp == SENT_F).all() and (cp == SENT_I).all() and not acc.counts.any() and not acc.loss.any()
    assert lib.lib().pbx_token_head_eval_parts(0) == 0 and lib.lib().pbx_token_head_eval_parts(257) == 2
    # the wrapper: shapes, dtypes and devices, before any launch
    w = lambda K, nb=1: torch.zeros(K, nb * CH, device="cuda")      # noqa: E731
    bias = lambda K: torch.zeros(K, device="cuda")                  # noqa: E731
    A = te.TaskEvalAccumulator
    badw = [dict(hs=[h], weight=w(0), bias=bias(0), acc=acc),                                   # K = 0
            dict(hs=[h], weight=w(17), bias=bias(17), acc=A(17, "cuda")),                       # K = 17
            dict(hs=[h] * 9, weight=w(3, 9), bias=bias(3), acc=acc),                            # nb = 9
            dict(hs=[], weight=w(3), bias=bias(3), acc=acc),                                    # nb = 0
            dict(hs=[h], weight=w(3), bias=bias(3), gterm=torch.zeros(B + 1, 3, device="cuda"), acc=acc),
            dict(hs=[h], weight=w(3), bias=bias(3), gterm=torch.zeros(B, 4, device="cuda"), acc=acc),
            dict(hs=[h], weight=w(3, 2), bias=bias(3), acc=acc),                                # W for two sources
            dict(hs=[h], weight=w(3), bias=bias(4), acc=acc),
            dict(hs=[h], weight=w(3), bias=bias(3), y=y.int(), acc=acc),                        # labels not int64
            dict(hs=[h], weight=w(3), bias=bias(3), y=y[:, :-1], acc=acc),
            dict(hs=[h], weight=w(3), bias=bias(3), y=y.cpu(), acc=acc),                        # another device
            dict(hs=[h], weight=w(3), bias=bias(3), acc=A(4, "cuda")),                          # accumulator of 4
            dict(hs=[h], weight=w(3), bias=bias(3), acc=A(3, "cpu")),
            dict(hs=[h.float()], weight=w(3), bias=bias(3), acc=acc)]                           # not bf16
    calls = []
    real = lib.call
    lib.call = lambda *a: calls.append(a)           # any launch attempt would be recorded
    try:
        for kw in badw:
            kw = dict(dict(gterm=None, y=y), **kw)
            with pytest.raises(ValueError):
                te.token_head_eval(**kw)
    finally:
        lib.call = real
    assert not calls
