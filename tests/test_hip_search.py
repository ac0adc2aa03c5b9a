"""GPU: ``pbx_search_topk`` (csrc/search.hip) alone, through ``ops.search.search_topk`` and the launcher.

* exact arithmetic: operands with integer entries in -2..2 make every score an exact fp32 integer with plentiful
  ties; values and indices must equal a CPU stable descending sort, at one split, three, and a split count that
  leaves splits with fewer than ``k`` rows (free slots, the merge);
* ordered databases (``s = r`` exactly): ascending scores send every row down the candidate path, descending
  ones only the first ``k``, an all-zero database ties everything;
* random cosine operands against fp64 scores of the same bf16 rows.  ``e`` = the larger of the maximum error
  of an independent fp32 torch evaluation and ``2^-24 max|s|``; ``tol = 16 e`` (the project's allowance for the
  MFMA's accumulation order);
* the optional stored scores: the selection is exact on the stored bits, which do not depend on the launch shape;
* repeatability, strided operands, byte offsets past 2^32, argument validation.

Measured on an MI355X (random cosine cases, the first eight shapes and every split count below): worst |value - fp64| / tol
0.104 (at 3 x 2500 x 1024, k = 64), and no unreturned row scored above a returned one (worst margin / (2 tol)
0.000)."""
import functools

import pytest
import torch

from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.ops.search import QUERY_TILE, search_topk, search_topk_torch

pytestmark = pytest.mark.gpu

BF, F64 = torch.bfloat16, torch.float64
# (nq, n, D, k): one tile and one row; a partial tile; D of three k-steps; several tiles; a partial last tile
# with the widest k; two staged chunks per tile; one query more than a workgroup's tile; n = 100 with k = 64; the
# kernel instance for 128 < D <= 256; a second chunk of a single k-step (D = 512 + 16)
SHAPES = [(1, 1, 16, 1), (5, 33, 16, 5), (33, 95, 48, 32), (70, 1000, 128, 10), (40, 4133, 512, 64),
          (3, 2500, 1024, 64), (QUERY_TILE + 1, 300, 32, 7), (5, 100, 64, 64), (9, 200, 208, 12), (4, 150, 528, 9)]


def _short_splits(n, k):
    """A split count that leaves splits with fewer than k rows: n = 100, k = 64 at S = 4 (32 rows a split, the last
    4); elsewhere two more splits than tiles, so the last two are empty."""
    return 4 if (n, k) == (100, 64) else (n + 31) // 32 + 2


def _stable(s, k):
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    return v[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def _exact_case(nq, n, D, k):
    """Integer operands, their exact scores and the stable top-k: computed once on the CPU, only read."""
    g = torch.Generator().manual_seed(nq * 1000003 + n * 101 + D)
    q = torch.randint(-2, 3, (nq, D), generator=g).to(BF)
    x = torch.randint(-2, 3, (n, D), generator=g).to(BF)
    s = q.float() @ x.float().t()                       # small integers: exact in any order
    v, i = _stable(s, k)
    return q.cuda(), x.cuda(), v, i, s


@functools.lru_cache(maxsize=None)
def _cosine_case(nq, n, D):
    g = torch.Generator().manual_seed(nq * 7919 + n * 31 + D)
    q = torch.randn(nq, D, generator=g)
    x = torch.randn(n, D, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).to(BF)
    x = (x / x.norm(dim=1, keepdim=True)).to(BF)
    s64 = q.to(F64) @ x.to(F64).t()
    s32 = q.float() @ x.float().t()
    e = max(float((s32.to(F64) - s64).abs().max()), 2.0 ** -24 * float(s64.abs().max()))
    return q.cuda(), x.cuda(), s64, 16 * e


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_scores_equal_stable_sort(shape):
    nq, n, D, k = shape
    q, x, v_ref, i_ref, s = _exact_case(*shape)
    if n > k:                                            # the tie rule is exercised, not assumed
        sv = torch.sort(s, dim=1, descending=True).values
        tied = int((sv[:, k - 1] == sv[:, k]).sum())
        print(f"{shape}: {tied} of {nq} query rows tie across the k-th place")
        assert tied > 0 or nq * n < 200
    for S in (1, 3, _short_splits(n, k), None):
        v, i = search_topk(q, x, k, splits=S)
        assert v.dtype == torch.float32 and i.dtype == torch.int32 and tuple(v.shape) == tuple(i.shape) == (nq, k)
        assert torch.equal(i.cpu(), i_ref), (shape, S)
        assert torch.equal(v.cpu(), v_ref), (shape, S)


def test_split_lists_and_free_slots():
    """The launcher's own output at n = 100, k = 64, S = 4: splits of 32, 32, 32 and 4 rows, each list the
    stable order of its range, the free slots -FLT_MAX / INT32_MAX."""
    nq, n, D, k = 5, 100, 64, 64
    q, x, _, _, s = _exact_case(nq, n, D, k)
    pval = torch.full((nq, 4, k), 7.0, device="cuda")
    pidx = torch.full((nq, 4, k), 7, dtype=torch.int32, device="cuda")
    _launch(q, x, k, 4, pval, pidx)
    pval, pidx = pval.cpu(), pidx.cpu()
    for j, (a, b) in enumerate(((0, 32), (32, 64), (64, 96), (96, 100))):
        v, i = _stable(s[:, a:b], b - a)
        assert torch.equal(pval[:, j, :b - a], v) and torch.equal(pidx[:, j, :b - a], i + a)
        assert (pval[:, j, b - a:] == -torch.finfo(torch.float32).max).all()
        assert (pidx[:, j, b - a:] == 2 ** 31 - 1).all()


def _launch(q, x, k, S, pval, pidx, scores=None, order=0):
    _lib.call("pbx_search_topk", q.data_ptr(), q.stride(0), x.data_ptr(), x.stride(0), q.shape[0], x.shape[0],
              q.shape[1], k, S, pval.data_ptr(), pidx.data_ptr(), _lib.ptr(scores),
              0 if scores is None else scores.stride(0), order, _lib.stream_ptr(q.device))


@pytest.mark.parametrize("S", [1, 5])
def test_ordered_databases(S):
    n, k = 20000, 64
    r = torch.arange(n)
    x = torch.zeros(n, 16)
    x[:, 0], x[:, 1] = r // 128, r % 128
    qv = torch.zeros(16)
    qv[0], qv[1] = 128, 1
    q = torch.stack([qv, -qv]).to(BF).cuda()             # query 0: s = r (ascending), query 1: s = -r
    assert torch.equal(x.to(BF).float(), x)              # the operands are exact in bf16
    v, i = search_topk(q, x.to(BF).cuda(), k, splits=S)
    v, i = v.cpu(), i.cpu()
    top = torch.arange(n - 1, n - 1 - k, -1)
    assert torch.equal(i[0].long(), top) and torch.equal(v[0], top.float())
    assert torch.equal(i[1].long(), torch.arange(k)) and torch.equal(v[1], -torch.arange(k).float())
    v, i = search_topk(q, torch.zeros(n, 16, dtype=BF, device="cuda"), k, splits=S)    # everything ties
    assert torch.equal(i.cpu().long(), torch.arange(k).expand(2, -1)) and not v.cpu().any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_cosine_against_fp64(shape):
    nq, n, D, k = shape
    q, x, s64, tol = _cosine_case(nq, n, D)
    tv, ti = search_topk_torch(q.cpu(), x.cpu(), k)
    worst_v = worst_m = 0.0
    for name, (v, i) in {"S=1": search_topk(q, x, k, splits=1), "S=3": search_topk(q, x, k, splits=3),
                         "S=short": search_topk(q, x, k, splits=_short_splits(n, k)),
                         "torch": (tv, ti)}.items():
        v, i = v.cpu(), i.cpu().long()
        assert int(i.min()) >= 0 and int(i.max()) < n, name
        assert all(len(set(row)) == k for row in i.tolist()), name                    # distinct
        at = s64.gather(1, i)
        err = float((v.to(F64) - at).abs().max())
        assert err <= tol, (name, err, tol)
        assert (v[:, :-1] >= v[:, 1:]).all(), name                                     # non-increasing
        eq = v[:, :-1] == v[:, 1:]
        assert (i[:, :-1][eq] < i[:, 1:][eq]).all(), name                              # equal neighbours: ascending
        rest = s64.clone()
        rest.scatter_(1, i, float("-inf"))
        margin = float((rest.max(dim=1).values - v.to(F64).min(dim=1).values).clamp(min=0).max()) if n > k else 0.0
        assert margin <= 2 * tol, (name, margin, tol)
        if name != "torch":
            worst_v, worst_m = max(worst_v, err / tol), max(worst_m, margin / (2 * tol))
    print(f"{shape}: tol {tol:.3e} worst |value - fp64| / tol {worst_v:.3f} worst unreturned margin / (2 tol) "
          f"{worst_m:.3f}")


def test_stored_scores_are_what_the_selection_used():
    nq, n, D, k = 40, 4133, 512, 64
    q, x, _, _ = _cosine_case(nq, n, D)
    SENT = -12345.0
    mats = {}
    for S in (1, 3, 7):
        buf = torch.full((nq + 3, n + 5), SENT, device="cuda")
        v, i = search_topk(q, x, k, splits=S, scores=buf[:nq, :n])
        b = buf.cpu()
        assert (b[nq:] == SENT).all() and (b[:, n:] == SENT).all()      # nothing outside [nq, n] is written
        mats[S] = b[:nq, :n].contiguous()
        sv, si = _stable(mats[S], k)
        assert torch.equal(i.cpu(), si)
        assert torch.equal(v.cpu().view(torch.int32), sv.view(torch.int32))
    assert torch.equal(mats[1].view(torch.int32), mats[3].view(torch.int32))
    assert torch.equal(mats[1].view(torch.int32), mats[7].view(torch.int32))
    few = torch.empty((7, n), device="cuda")                             # a prefix of the queries: another tile fill
    search_topk(q[:7], x, k, splits=2, scores=few)
    assert torch.equal(few.cpu().view(torch.int32), mats[1][:7].view(torch.int32))
    # and the matrix is the score: within the MFMA allowance of fp64
    _, _, s64, tol = _cosine_case(nq, n, D)
    assert float((mats[1].to(F64) - s64).abs().max()) <= tol


def test_stored_scores_with_exact_operands_and_both_grid_orders():
    nq, n, D, k = QUERY_TILE + 1, 300, 32, 7
    q, x, v_ref, i_ref, s = _exact_case(nq, n, D, k)
    for order in (0, 1):
        out = torch.empty((nq, n), device="cuda")
        v, i = search_topk(q, x, k, splits=3, scores=out, order=order)
        assert torch.equal(out.cpu(), s) and torch.equal(i.cpu(), i_ref) and torch.equal(v.cpu(), v_ref)


def test_two_launches_into_different_buffers_are_bitwise_equal():
    nq, n, D, k = 70, 1000, 128, 10
    q, x, _, _ = _cosine_case(nq, n, D)
    outs = []
    for fill in (0.0, float("nan")):
        pval = torch.full((nq, 3, k), fill, device="cuda")
        pidx = torch.full((nq, 3, k), -5 if fill == 0.0 else 99, dtype=torch.int32, device="cuda")
        _launch(q, x, k, 3, pval, pidx)
        outs.append((pval.cpu(), pidx.cpu()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1], outs[1][1])


def test_strided_operands():
    nq, n, D, k = 33, 95, 48, 32
    q, x, v_ref, i_ref, _ = _exact_case(nq, n, D, k)
    qs = torch.full((nq, D + 8), 3.0, dtype=BF, device="cuda")
    xs = torch.full((n, D + 40), 3.0, dtype=BF, device="cuda")
    qs[:, :D], xs[:, :D] = q, x
    qv, xv = qs[:, :D], xs[:, :D]
    assert qv.stride(0) == D + 8 and xv.stride(0) == D + 40
    v, i = search_topk(qv, xv, k, splits=2)
    assert torch.equal(i.cpu(), i_ref) and torch.equal(v.cpu(), v_ref)
    # a row stride that breaks the 16-byte alignment is copied, not refused
    xo = torch.full((n, D + 4), 3.0, dtype=BF, device="cuda")
    xo[:, :D] = x
    v, i = search_topk(q, xo[:, :D], k)
    assert torch.equal(i.cpu(), i_ref) and torch.equal(v.cpu(), v_ref)


def test_byte_offsets_past_4gib():
    n, D, k, nq = 4_200_000, 512, 8, 32
    assert n * D * 2 > 2 ** 32
    x = torch.zeros(n, D, dtype=BF, device="cuda")
    planted = {n - 1: 3.0, n - 1000: 5.0, n - 417: 4.0}                 # row -> x[row, 0]
    for row, val in planted.items():
        x[row, 0] = val
    q = torch.zeros(nq, D, dtype=BF)
    q[:, 0] = torch.arange(1, nq + 1).float()                           # query j: s = (j + 1) x[r, 0]
    order = sorted(planted, key=lambda row: -planted[row])
    want_i = torch.tensor(order + list(range(k - 3)), dtype=torch.int32).expand(nq, -1)
    want_v = torch.zeros(nq, k)
    want_v[:, :3] = torch.arange(1, nq + 1).float()[:, None] * torch.tensor([planted[row] for row in order])
    for S in (None, 7):
        v, i = search_topk(q.cuda(), x, k, splits=S)
        assert torch.equal(i.cpu(), want_i) and torch.equal(v.cpu(), want_v), S


def test_invalid_arguments_raise_before_any_launch():
    def ops(nq, n, D):
        return torch.zeros(nq, D, dtype=BF, device="cuda"), torch.zeros(n, D, dtype=BF, device="cuda")
    for nq, n, D, k, S in ((2, 100, 24, 1, 1), (2, 100, 1040, 1, 1), (2, 100, 64, 65, 1), (2, 10, 64, 11, 1),
                           (2, 100, 64, 64, 257), (2, 100, 64, 1, 0)):
        q, x = ops(nq, n, D)
        with pytest.raises(ValueError):
            search_topk(q, x, k, splits=S)
        # the launcher refuses the same values itself (hipErrorInvalidValue, nothing launched: outputs untouched)
        pval = torch.full((nq, max(S, 1), k), 7.0, device="cuda")
        pidx = torch.full((nq, max(S, 1), k), 7, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.HipError, match="pbx_search_topk"):
            _launch(q, x, k, S, pval, pidx)
        torch.cuda.synchronize()
        assert (pval == 7.0).all() and (pidx == 7).all()
    q, x = ops(2, 100, 64)
    with pytest.raises(ValueError):
        search_topk(q, x[:, :32], 1)
    with pytest.raises(ValueError):
        search_topk(q, x, 1, scores=torch.zeros(2, 99, device="cuda"))
    with pytest.raises(ValueError):
        search_topk(q.float(), x, 1)
    with pytest.raises(ValueError):
        search_topk(q.cpu(), x.cpu(), 1)
