"""GPU: the two pretraining heads stage by stage, per element, against the fp64 oracles of tests/head_oracles.py.

The launchers are called directly (``_lib.call``): ``pbx_local_head3_a/_b/_c`` hand every intermediate of the
five-pass local head to the test (Z, the per-chunk partials, (M, 1/S) or raw (M, S), the partials of T, T, the loss
partials), so each stage is compared with fp64 from the tensors the kernel itself stored for the stage before;
``pbx_local_head_fused`` (one launch, B <= 2048, the TPW 2 / 4 / 8 instantiations) has only outputs, compared with
the whole chain; ``pbx_go_head_fused`` is the ``EPI_GO`` epilogue of ``csrc/gemm.hip``; ``HeadsLossFn`` is run end to
end with an incoming gradient of 1 and of 2.5.  A batch axis shared by two "ranks" is played on one GPU (raw = 1,
host merge of the (M, S) images as ``parallel/batch_softmax.merge_head_stats`` does it, T summed).

The condition is ``|X_k - X_64| <= free + 16 e32`` per element (head_oracles' docstring says what ``free`` and the
floors of e32 are; no tolerance is a constant picked in advance).  tests/test_head_oracles.py shows on the CPU that
the oracle is right, that an honest fp32 kernel meets these conditions on exactly these cases, and that seventeen
kinds of wrong kernel do not.  Every output lives in a ``Buf`` (16 guard rows of a NaN sentinel): guards stay
untouched, no sentinel remains where the contract says "written", a second launch repeats bitwise.

Three things had to be argued (head_oracles says where): a sample whose weight is 0 at every position has G = 0 but
still receives dZ = -P T, because the softmax couples the batch, so exact zeros are asserted for the all-masked
POSITION only and the masked sample is held to the element-wise condition; at B = 1 the five-pass form stores not 0
but the exact rounding residual of G (the compiler contracts ``coef * x - T`` into one fma), at most 2^-24 |G|, which is
what is asserted (measured: 0.12 of that bound); and dZ = P G - P T is itself a cancelling sum, so its yardstick and
that of its column sums are floored by 2^-24 (|P G| + |P T|), the only thing that bounds them where they cancel to 0.

``PBX_HEADS_EXACT_REPORT=path`` writes each tensor's largest err / e32 over the session, the e32 values and every
derived intrinsic term that was needed (profiles/r25/heads_exact.txt)."""
import os

import pytest
import torch

import head_oracles as ho
from head_oracles import VP
from test_hip_conv_exact import exact_library
from test_hip_global_exact import Buf

from proteinbert_pytorch_replication_amd.ops import _lib, gemm as gemm_ops, global_track as gt

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
LEDGER = ho.HeadLedger()


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    out = os.environ.get("PBX_HEADS_EXACT_REPORT")
    if out and LEDGER.worst:
        with open(out, "w") as fh:
            fh.write("largest err / e32 per checked tensor over all cases of tests/test_hip_heads_exact.py\n"
                     "(assertion: excess over the free term <= 16 e32; e32 in units of its floors where one applies;\n"
                     " (bf16) rows: the excess over the half ulp)\n")
            for n, r in LEDGER.worst.items():
                fh.write(f"{n:<34s} {r:8.3f}\n")
            fh.write("\nlargest e32 per tensor, and every derived intrinsic term that was needed\n")
            for n, v in LEDGER.notes.items():
                fh.write(f"{n:<46s} {v:.4g}\n")


def _dev():
    return torch.device("cuda")


def _st():
    return _lib.stream_ptr(_dev())


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    for n in a:
        assert torch.equal(_bits(a[n].full), _bits(b[n].full)), f"{n}: a second launch differs"


def _cpu(bufs):
    return {n: b.v.detach().cpu().clone() for n, b in bufs.items()}


def _written(bufs, V, A=None):
    """Guards untouched everywhere; finite values where the contract says written (columns v >= V of the partials
    and statistics are unspecified)."""
    for n, b in bufs.items():
        assert b.guards_ok(), f"{n}: rows past the end were written"
        v = b.v
        if n in ("part", "MS", "tpart"):
            v = v[..., :V, :]
        if n == "T":
            v = v[..., :V, 0]
        assert bool(torch.isfinite(v.float()).all()), f"{n}: a sentinel remains where the kernel writes"


def _local_dev(c):
    d = _dev()
    return dict(h=c["h"].to(d), wo=c["wo"].to(d).contiguous(), bo=c["bo"].to(d), y=c["y"].to(d).contiguous(),
                w=c["w"].to(d).contiguous())


# ---- the five-pass form ---------------------------------------------------------------------------------------
def five_bufs(B, L, V):
    nch, nt = ho.nchunks(B), ho.ntiles(B, L)
    assert _lib.lib().pbx_local_head3_tiles(B, L) == nt
    return dict(Z=Buf(B * L, VP), part=Buf(nch, L, VP, 2), MS=Buf(L, VP, 2), tpart=Buf(nch, L, VP, 2), T=Buf(L, VP, 2),
                loss_part=Buf(nt), dz=Buf(B * L, VP, dt=BF16), dh=Buf(B * L, ho.CH, dt=BF16), dbo_part=Buf(nt, V))


def stage_a(d, b, B, L, V, raw):
    _lib.call("pbx_local_head3_a", d["h"].data_ptr(), d["wo"].data_ptr(), d["bo"].data_ptr(), b["Z"].full.data_ptr(),
              b["part"].full.data_ptr(), b["MS"].full.data_ptr(), int(raw), B, L, V, _st())
    torch.cuda.synchronize()


def stage_b(d, b, ms, B, L, V):
    _lib.call("pbx_local_head3_b", b["Z"].full.data_ptr(), ms.data_ptr(), d["y"].data_ptr(), d["w"].data_ptr(),
              b["tpart"].full.data_ptr(), b["loss_part"].full.data_ptr(), b["T"].full.data_ptr(), B, L, V, _st())
    torch.cuda.synchronize()


def stage_c(d, b, ms, T, B, L, V):
    _lib.call("pbx_local_head3_c", b["Z"].full.data_ptr(), ms.data_ptr(), T.data_ptr(), d["y"].data_ptr(),
              d["w"].data_ptr(), d["wo"].data_ptr(), d["bo"].data_ptr(), b["dh"].full.data_ptr(), b["dz"].full.data_ptr(),
              b["dbo_part"].full.data_ptr(), B, L, V, _st())
    torch.cuda.synchronize()


def merged(raws):
    """The host merge of raw (M, S) images [L, 32, 2] as batch_softmax.merge_max_sum / merge_head_stats do it:
    mg = max_r M_r, sg = sum_r S_r exp(M_r - mg), then (mg, 1 / sg) (0 where sg == 0)."""
    mg = torch.stack([r[..., 0] for r in raws]).max(dim=0).values
    sg = sum(r[..., 1] * torch.exp(r[..., 0] - mg) for r in raws)
    inv = torch.where(sg > 0, 1.0 / sg.clamp_min(torch.finfo(F32).tiny), torch.zeros_like(sg))
    return torch.stack([mg, inv], dim=-1).contiguous()


def run_five(d, B, L, V, raw):
    b = five_bufs(B, L, V)
    stage_a(d, b, B, L, V, raw)
    ms = merged([b["MS"].v]) if raw else b["MS"].v
    stage_b(d, b, ms, B, L, V)
    stage_c(d, b, ms, b["T"].v, B, L, V)
    return b, ms


def _five_case(shape, regime, raw, tag):
    c = ho.make_local(*shape, regime)
    B, L, V = shape
    d = _local_dev(c)
    b, ms = run_five(d, B, L, V, raw)
    _written(b, V)
    b2, _ = run_five(d, B, L, V, raw)
    _same(b, b2)
    k = _cpu(b)
    k["dh"] = k["dh"].reshape(B, L, ho.CH)
    ho.check_five(c, k, raw=raw, MS_used=ms.cpu() if raw else None, ledger=LEDGER, tag=tag)
    if B > 2048 and not raw:
        # production routes this size to the same three launchers, with one row of bias partials per tile
        assert _lib.lib().pbx_local_head_fused_pp(B) == 0
        slot = torch.zeros(1, device=_dev())
        dh, dz, dbo_part = gt.local_head_forward(d["h"], d["wo"], d["bo"], d["y"], d["w"], slot)
        torch.cuda.synchronize()
        assert dbo_part.shape == (ho.ntiles(B, L), V)
        assert torch.equal(_bits(dz), _bits(b["dz"].v)) and torch.equal(_bits(dh.reshape(B * L, -1)), _bits(b["dh"].v))


@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("shape,regime", ho.FIVE_CASES)
def test_five_pass_stagewise(shape, regime, raw):
    _five_case(shape, regime, bool(raw), f"five.{regime}" + (".raw" if raw else ""))


def test_five_pass_exact_library():
    with exact_library():
        _five_case((17, 33, 26), "plain", False, "five.plain")
    assert _lib.gelu_mode() != "custom"


def test_shared_batch_axis_two_shards():
    """(34, 33, 26) as two ranks of 17: each shard against the oracle of the FULL batch with its own 1 / (17 * 33)."""
    shape, Bs = ho.SHARED_CASE
    B, L, V = shape
    c = ho.make_local(*shape, "plain")
    shards = [ho.shard_of(c, lo, Bs) for lo in range(0, B, Bs)]
    ds = [_local_dev(s) for s in shards]
    bs = [five_bufs(Bs, L, V) for _ in shards]
    for d, b in zip(ds, bs):
        stage_a(d, b, Bs, L, V, True)
    ms = merged([b["MS"].v for b in bs])
    for d, b in zip(ds, bs):
        stage_b(d, b, ms, Bs, L, V)
    T = (bs[0]["T"].v + bs[1]["T"].v).contiguous()
    for d, b in zip(ds, bs):
        stage_c(d, b, ms, T, Bs, L, V)
    for i, (s, b) in enumerate(zip(shards, bs)):
        _written(b, V)
        k = _cpu(b)
        k["dh"] = k["dh"].reshape(Bs, L, ho.CH)
        ho.check_five(s, k, raw=True, Bc=Bs, MS_used=ms.cpu(), T_used=T.cpu(), ledger=LEDGER, tag="shard.stage")
        ho.check_shard(c, i * Bs, k, Bs, ledger=LEDGER, tag="shard.full")


# ---- the one-launch form ----------------------------------------------------------------------------------------
def run_fused(d, B, L, V):
    b = dict(dh=Buf(B * L, ho.CH, dt=BF16), dz=Buf(B * L, VP, dt=BF16), dbo_part=Buf(L, V), loss_part=Buf(L))
    _lib.call("pbx_local_head_fused", d["h"].data_ptr(), d["wo"].data_ptr(), d["bo"].data_ptr(), d["y"].data_ptr(),
              d["w"].data_ptr(), b["dh"].full.data_ptr(), b["dz"].full.data_ptr(), b["dbo_part"].full.data_ptr(),
              b["loss_part"].full.data_ptr(), B, L, V, _st())
    torch.cuda.synchronize()
    return b


def _fused_case(shape, regime, tag, routed=True):
    c = ho.make_local(*shape, regime)
    B, L, V = shape
    assert _lib.lib().pbx_local_head_fused_pp(B) == 1
    d = _local_dev(c)
    b = run_fused(d, B, L, V)
    _written(b, V)
    _same(b, run_fused(d, B, L, V))
    k = _cpu(b)
    k = dict(dz=k["dz"], dh=k["dh"].reshape(B, L, ho.CH), dbo_pos=k["dbo_part"], loss_pos=k["loss_part"])
    ho.check_fused(c, k, ledger=LEDGER, tag=tag)
    if routed:
        # production routes this size to the same launcher, with L rows of bias partials
        slot = torch.zeros(1, device=_dev())
        dh, dz, dbo_part = gt.local_head_forward(d["h"], d["wo"], d["bo"], d["y"], d["w"], slot)
        torch.cuda.synchronize()
        assert dbo_part.shape == (L, V)
        assert torch.equal(_bits(dz), _bits(b["dz"].v)) and torch.equal(_bits(dh.reshape(B * L, -1)), _bits(b["dh"].v))


@pytest.mark.parametrize("shape,regime", ho.FUSED_CASES)
def test_one_launch_per_element(shape, regime):
    _fused_case(shape, regime, f"fused.{regime}")


def test_one_launch_exact_library():
    with exact_library():
        _fused_case((33, 5, 26), "plain", "fused.plain", routed=False)
    assert _lib.gelu_mode() != "custom"


# ---- the GO head --------------------------------------------------------------------------------------------------
def run_go(c):
    d = _dev()
    B, A, G = c["B"], c["A"], c["G"]
    tr, tc = ho.go_tiles(B, A)
    assert gemm_ops.go_head_parts(B, A) == tr * tc
    x, wa, ba = c["x"].to(d).contiguous(), c["wa"].to(d).contiguous(), c["ba"].to(d)
    y = c["ypad"].to(d).contiguous()
    wrow = None if "wfull" in c else c["wrow"].to(d).contiguous()
    wfull = c["wfull"].to(d).contiguous() if "wfull" in c else None
    b = dict(dz=Buf(B, c["lddz"], dt=BF16), dbias_part=Buf(tr, A), loss_part=Buf(tr * tc))
    _lib.call("pbx_go_head_fused", x.data_ptr(), x.stride(0), wa.data_ptr(), wa.stride(0), ba.data_ptr(), y.data_ptr(),
              c["ldy"], _lib.ptr(wrow), _lib.ptr(wfull), b["dz"].full.data_ptr(), c["lddz"], b["dbias_part"].full.data_ptr(),
              b["loss_part"].full.data_ptr(), B, A, G, _st())
    torch.cuda.synchronize()
    return b


def _go_case(case, tag):
    B, A, G, ldy, lddz, wfull = case
    c = ho.make_go_case(B, A, G, ldy, lddz, wfull)
    b = run_go(c)
    _written(b, 0)
    _same(b, run_go(c))
    ho.check_go(c, _cpu(b), ledger=LEDGER, tag=tag)


@pytest.mark.parametrize("case", ho.GO_CASES)
def test_go_head_per_element(case):
    _go_case(case, "go")


def test_go_head_exact_library():
    with exact_library():
        _go_case(ho.GO_CASES[2], "go")
    assert _lib.gelu_mode() != "custom"


def test_go_head_real_width_through_go_head_forward():
    """(129, 8943, 512) through ``go_head_forward``: its padded dz buffer, its bias partials and its loss slot."""
    B, A, G = ho.GO_REAL
    c = ho.make_go_case(B, A, G, A, gt.padded_cols(A))
    d = _dev()
    slot = torch.full((1,), float("nan"), device=d)
    wa = c["wa"].to(d).float()
    w_g = c["wrow"].to(d)[:, None].expand(B, A)        # expanded on the device: training's per-row weight route
    assert w_g.stride(1) == 0
    dz, dba, _ = gt.go_head_forward(c["x"].to(d), wa, c["ba"].to(d), c["y"].to(d), w_g, slot)
    torch.cuda.synchronize()
    base = dz._base if dz._base is not None else dz
    assert base.shape == (B, gt.padded_cols(A)) and dba.shape == ((B + 127) // 128, A)
    o64 = ho.st_go(c["x"], c["wa"], c["ba"], c["y"], c["w"], F64)
    o32 = ho.st_go(c["x"], c["wa"], c["ba"], c["y"], c["w"], F32)
    # the loss partials stay inside go_head_forward: the slot is their fixed-order sum, checked as one sum below
    k = dict(dz=base.cpu(), dbias_part=dba.cpu())
    ho.check_go(c, k, ledger=LEDGER, tag="go.real", ref=(o64, o32))
    ho.cmp(few=True, name="go.real.loss", xk=slot.cpu().reshape(()), x64=o64["loss_tile"].sum(), x32=o32["loss_tile"].sum(),
           floor=ho.U24 * o64["loss_tile_abs"].sum(), intr=ho.logf_term(o64["loss_tile_abs"].sum()), ledger=LEDGER)


# ---- HeadsLossFn end to end -------------------------------------------------------------------------------------
def _run_heads(cl, cg, scale, unit=False):
    d = _dev()
    P = torch.nn.Parameter
    wo, bo = P(cl["wo"].to(d)), P(cl["bo"].to(d))
    wa, ba = P(cg["wa"].to(d).float()), P(cg["ba"].to(d))
    h = cl["h"].to(d).requires_grad_(True)
    g = cg["x"].to(d).float().requires_grad_(True)
    w_g = cg["wrow"].to(d)[:, None].expand(cg["B"], cg["A"])     # the per-row weight route of go_head_forward
    assert w_g.stride(1) == 0
    total, _ = gt.HeadsLossFn.apply(h, g, cg["x"].to(d), wo, bo, wa, ba, cl["y"].to(d), cg["y"].to(d), cl["w"].to(d),
                                    w_g)
    if unit:
        with gt.unit_loss_grad():
            total.backward()
    else:
        (total if scale == 1.0 else scale * total).backward()
    torch.cuda.synchronize()
    return dict(total=total.detach().cpu(), dh=h.grad.cpu(), dg=g.grad.cpu(), dWo=wo.grad.cpu(), dbo=bo.grad.cpu(),
                dWa=wa.grad.cpu(), dba=ba.grad.cpu())


def test_heads_loss_fn_end_to_end():
    """dWo, dbo, dWa, dba, dh, dg per element with an incoming gradient of 1 and of 2.5 (the ``scale`` branch); at 1
    the unit-gradient shortcut gives the same bits."""
    B, L, A, G = ho.E2E_CASE
    cl, cg = ho.make_local(B, L, 26), ho.make_go_case(B, A, G)
    one = _run_heads(cl, cg, 1.0)
    ho.check_e2e(cl, cg, 1.0, one, ledger=LEDGER, tag="e2e.x1")
    unit = _run_heads(cl, cg, 1.0, unit=True)
    for n in one:
        assert torch.equal(_bits(one[n]), _bits(unit[n])), f"{n}: _UNIT_LOSS_GRAD changes the result at scale 1"
    got = _run_heads(cl, cg, 2.5)
    got.pop("total")
    ho.check_e2e(cl, cg, 2.5, got, ledger=LEDGER, tag="e2e.x2.5")
