"""GPU: ``pbx_ln_linear_fwd``, ``pbx_ln2_linear_bwd`` (with ``ln2_consts_kernel``), ``pbx_embed_fwd`` and
``pbx_embed_bwd`` of ``ops/csrc/ln.hip`` stage by stage against the fp64 oracles of tests/ln_oracles.py.

The launchers are called directly (``_lib.call``), so every stored tensor is in the test's hands: each stage is
compared per element with fp64 from the tensors the kernel was given or itself stored for the stage before.  No
tolerance is a constant: 16 x the measured error of an fp32 torch evaluation of the same stage, half a bf16 ulp for a
bf16 store, the documented 1.5e-7 of the A&S erf core in the exact build, and for the roundings the kernels never
store (the bf16 h1 operand of both kernels, the backward's dpre) an admissible interval whose width is carried into
the stages behind it.  tests/test_ln_oracles.py shows on the CPU that the oracle is right, that these conditions
reject twelve kinds of wrong kernel, and that the intervals stay narrow on every case used here.

Every output has 16 guard rows filled with a NaN sentinel (``test_hip_global_exact.Buf``): guards must stay
untouched, no sentinel may remain below, and a second launch repeats bitwise where the kernel has a single writer.
The shapes are chosen by what ONE workgroup walks, derived from the device's CU count as the launchers do
(``ln_oracles.fwd_groups`` / ``bwd_grid``); :func:`test_walks_on_this_device` asserts the walks they are meant to
produce, so that another CU count fails loudly instead of covering less.  ``PBX_LN_EXACT_REPORT=path`` writes each
tensor's largest err / e32 over the session, the e32 of the hidden roundings, the ambiguous shares, the drift / rms
ratios and the M2 ratios (profiles/r23/ln_exact.txt)."""
import os

import pytest
import torch

import ln_oracles as lo
from ln_oracles import C, EPS, PB, V
from test_hip_conv_exact import exact_library
from test_hip_global_exact import Buf

from proteinbert_pytorch_replication_amd.ops import _lib

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LEDGER = lo.ConvLedger()
SINGLE = ("consts", "dh1", "sums1")             # the backward's outputs with a single writer


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    out = os.environ.get("PBX_LN_EXACT_REPORT")
    if out and LEDGER.worst:
        with open(out, "w") as fh:
            fh.write("largest err / e32 per checked tensor over all cases of tests/test_hip_ln_exact.py\n"
                     "(assertion: err <= 16 e32 beyond the free terms; bf16 rows: excess over the half ulp)\n")
            for n, r in LEDGER.worst.items():
                fh.write(f"{n:<40s} {r:8.3f}\n")
            fh.write("\nlargest e32 of the hidden roundings, ambiguous shares, drift / rms and M2 ratios\n")
            for n, r in LEDGER.notes.items():
                fh.write(f"{n:<48s} {r:10.4g}\n")


def _dev():
    return torch.device("cuda")


def _st():
    return _lib.stream_ptr(_dev())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _to_dev(c):
    return {n: (v.to(_dev()).contiguous() if torch.is_tensor(v) else v) for n, v in c.items()}


def _mode():
    mode = _lib.gelu_mode()
    assert mode in ("fitted", "exact")
    return mode


def _tag(base):
    return base + ("|exact" if _lib.gelu_mode() == "exact" else "")


def _written(bufs, skip=()):
    for n, b in bufs.items():
        if b is not None and n not in skip:
            b.assert_written(n)


def _same_bits(a, b, names):
    for n in names:
        if a.get(n) is not None:
            it = torch.int16 if a[n].dt == BF16 else torch.int32
            assert torch.equal(a[n].v.view(it), b[n].v.view(it)), f"{n}: two launches differ"


# ---- the walks ----------------------------------------------------------------------------------------------
FWD_LONG = (4096, 4090)
BWD_CASES = [(1, 512), (16, 512), (17, 512), (37, 512), (33, 511), (2, 33), (80, 64), (3, 514), (17, 515), (2, 1026)]
BWD_DET = [(37, 512), (17, 515), (80, 64)]
BWD_MODES = [(17, 512), (3, 514)]


def fwd_walk_batches(L):
    """B in {g, g D + 1, g (2 D + 1) - 1, g (2 D + 1)}: one workgroup walks 1, {D, D + 1}, {2 D, 2 D + 1}, 2 D + 1
    samples (g the launcher's sample groups at a large batch, D the ring depth of ln.hip)."""
    D = _lib.lib().pbx_ln_fwd_ring()
    g = lo.fwd_groups(10 ** 6, L, _cus())
    return D, g, [g, g * D + 1, g * (2 * D + 1) - 1, g * (2 * D + 1)]


def test_walks_on_this_device():
    """The shapes of this file produce the walks they are meant to on this device (they are stated for 256 CUs)."""
    cus = _cus()
    for L in FWD_LONG:
        D, g, Bs = fwd_walk_batches(L)
        walks = [lo.fwd_walks(B, L, cus) for B in Bs]
        print(f"forward L={L}: CUs={cus} groups={g} D={D} batches={Bs} walks={walks}")
        assert Bs == [4, 5, 11, 12], "tests/test_ln_oracles.py asserts the conditions on these batch sizes"
        assert walks == [[1], sorted({D, D + 1}), [2 * D, 2 * D + 1], [2 * D + 1]]
    # backward: (pairs workgroup 0 walks, its 16-sample chunks, sample splits)
    want = {(1, 512, 0): ([0], 1, 1), (16, 512, 0): ([0], 1, 1), (17, 512, 0): ([0], 2, 1), (37, 512, 0): ([0], 3, 1),
            (33, 511, 0): ([0], 3, 1), (2, 33, 0): ([0], 1, 1), (80, 64, 0): ([0], 1, 5), (80, 64, 1): ([0], 5, 1),
            (3, 514, 0): ([0, 256], 1, 1), (17, 515, 0): ([0, 256], 2, 1), (17, 515, 1): ([0, 256], 2, 1),
            (2, 1026, 0): ([0, 256, 512], 1, 1), (37, 512, 1): ([0], 3, 1)}
    assert {(B, L) for B, L, _ in want} == set(BWD_CASES)
    for (B, L, det), w in want.items():
        got = lo.bwd_walk(B, L, det, cus)
        gx, ns = lo.bwd_grid(B, L, det, cus)
        print(f"backward B={B} L={L} det={det}: grid ({gx}, {ns}) pairs {got[0]} chunks {got[1]} splits {got[2]}")
        assert got == w, (B, L, det, got, w)
        assert _lib.lib().pbx_ln2_bwd_slab_rows(B, L, det) == gx * ns


# ---- forward ------------------------------------------------------------------------------------------------
def launch_fwd(cd, with_pre=True):
    B, L = cd["B"], cd["L"]
    T2 = (L + PB - 1) // PB
    b = dict(pre_l=Buf(B * L, C, dt=BF16) if with_pre else None, s2=Buf(B * L, C, dt=BF16), st2=Buf(B * T2, 2))
    _lib.call("pbx_ln_linear_fwd", cd["s1"].data_ptr(), cd["st1"].data_ptr(), cd["st1"].shape[1], cd["BM1"],
              cd["g1"].data_ptr(), cd["be1"].data_ptr(), cd["wl"].data_ptr(), cd["bl"].data_ptr(),
              None if b["pre_l"] is None else b["pre_l"].full.data_ptr(), b["s2"].full.data_ptr(),
              b["st2"].full.data_ptr(), B, L, EPS, _st())
    torch.cuda.synchronize()
    return b


def _k_fwd(b, B, L):
    cpu = lambda n: b[n].v.detach().cpu().clone()  # noqa: E731
    return dict(pre_l=None if b["pre_l"] is None else cpu("pre_l").reshape(B, L, C), s2=cpu("s2").reshape(B, L, C),
                st2=cpu("st2").reshape(B, -1, 2))


def _forward_case(B, L, bm1=128, inference=False):
    mode = _mode()
    tag = _tag("fwd" if bm1 == 128 else f"fwd|bm{bm1}")
    c = lo.make_case(B, L, bm1, backward=False)
    cd = _to_dev(c)
    print(f"-- pbx_ln_linear_fwd B={B} L={L} BM1={bm1} T1={c['st1'].shape[1]} walks={lo.fwd_walks(B, L, _cus())} ({mode})")
    ref = lo.forward_ref(c, mode, LEDGER, None, tag)
    b = launch_fwd(cd)
    _written(b)
    lo.check_forward(c, _k_fwd(b, B, L), mode, LEDGER, None, tag, ref)
    _same_bits(b, launch_fwd(cd), ("pre_l", "s2", "st2"))
    if inference:                                            # pre_l = None: the same s2 and st2 bits
        bi = launch_fwd(cd, with_pre=False)
        _written(bi)
        _same_bits(b, bi, ("s2", "st2"))


@pytest.mark.parametrize("L", FWD_LONG)
@pytest.mark.parametrize("i", range(4))
def test_forward_sample_walks(L, i):
    """A workgroup walks 1, {D, D + 1}, {2 D, 2 D + 1} and 2 D + 1 samples; L = 4090: a last tile of 26 rows."""
    _forward_case(fwd_walk_batches(L)[2][i], L)


def test_forward_one_row_tile():
    """(L = 33, B = 1): the second tile has one row; without pre_l the same s2 and st2 bits."""
    _forward_case(1, 33, inference=True)


def test_forward_whole_tile():
    _forward_case(3, 64, inference=True)


@pytest.mark.parametrize("L", FWD_LONG)
def test_forward_first_block_partials(L):
    """BM1 = 4 (the first block's layout): T1 = 1024, 16 trips of the per-lane merge loop of wave_ln_stats; at
    L = 4090 the last partial holds 2 positions."""
    _forward_case(4, L, bm1=4)


@pytest.mark.parametrize("B,L,bm1", [(1, 33, 128), (5, 4090, 128), (4, 4090, 4)])
def test_forward_exact_library(B, L, bm1):
    with exact_library():
        _forward_case(B, L, bm1, inference=L == 33)
    assert _lib.gelu_mode() != "custom"


# ---- backward -----------------------------------------------------------------------------------------------
def launch_bwd(cd, det=0, slab="full", fold=1, consts=None):
    """pbx_ln2_linear_bwd into fresh sentinel-filled / preloaded buffers.  slab: "full" (the rows the launcher asks
    for), "small" (one row fewer: the atomic fallback) or None (atomics).  consts: a Buf of an earlier call
    (consts_ready = 1)."""
    B, L = cd["B"], cd["L"]
    TS1, TA = (L + 1) // 2, (L + PB - 1) // PB
    b = dict(dh1=Buf(B * L, C, dt=BF16), sums1=Buf(B * TS1, 2), consts=consts or Buf(B, 8), dgb=Buf(B, C))
    for n in lo.GRADS:
        b[n] = Buf(cd[n + "_0"].shape[0], *cd[n + "_0"].shape[1:], fill=cd[n + "_0"])
    rows = _lib.lib().pbx_ln2_bwd_slab_rows(B, L, det)
    srows = None if slab is None else (rows if slab == "full" else rows - 1)
    b["slab"] = None if slab is None else Buf(srows, C * C + C)
    _lib.call("pbx_ln2_linear_bwd", cd["dh2"].data_ptr(), cd["s2"].data_ptr(), cd["st2"].data_ptr(),
              cd["sums2"].data_ptr(), TA, cd["g2"].data_ptr(), cd["pre_l"].data_ptr(), cd["s1"].data_ptr(),
              cd["st1"].data_ptr(), cd["st1"].shape[1], cd["BM1"], cd["g1"].data_ptr(), cd["be1"].data_ptr(),
              cd["wl"].data_ptr(), b["consts"].full.data_ptr(), b["dh1"].full.data_ptr(), b["sums1"].full.data_ptr(),
              b["dg2"].full.data_ptr(), b["db2"].full.data_ptr(), b["dg1"].full.data_ptr(), b["db1"].full.data_ptr(),
              b["dwl"].full.data_ptr(), b["dbl"].full.data_ptr(), b["dgb"].full.data_ptr(), B, L, EPS,
              None if slab is None else b["slab"].full.data_ptr(), 0 if slab is None else srows, det, fold,
              0 if consts is None else 1, _st())
    torch.cuda.synchronize()
    # the slab: every row written when it is used, untouched when the launcher falls back to atomics
    if slab == "full":
        b["slab"].assert_written("slab")
    elif slab == "small":
        assert b["slab"].untouched(), "a slab one row too small was written to"
    if consts is None:
        assert b["dgb"].guards_ok() and bool((b["dgb"].v == 0).all()), "dgb_zero: not every row zeroed exactly"
    else:
        assert b["dgb"].untouched(), "consts_ready = 1: dgb_zero was written to"
    _written(b, skip=("slab", "dgb"))
    return b


def _got_bwd(b, B, L):
    got = {n: b[n].v.detach().cpu().clone() for n in (*SINGLE, *lo.GRADS)}
    got["dh1"], got["sums1"] = got["dh1"].reshape(B, L, C), got["sums1"].reshape(B, (L + 1) // 2, 2)
    return got


def _backward_base(B, L, det, tag):
    """The launcher's default form (slab, fold = 1) twice: constants, every output, bitwise repeats."""
    mode = _mode()
    c = lo.make_case(B, L)
    cd = _to_dev(c)
    print(f"-- pbx_ln2_linear_bwd B={B} L={L} det={det} walk={lo.bwd_walk(B, L, det, _cus())} ({mode})")
    b = launch_bwd(cd, det)
    got = _got_bwd(b, B, L)
    kb = lo.bwd_inputs(c)
    lo.check_consts(c, kb, got["consts"], LEDGER, None, tag)
    ref = lo.backward_ref(c, kb, got["consts"], mode, LEDGER, None, tag)
    lo.check_backward(c, got, ref, LEDGER, None, tag)
    _same_bits(b, launch_bwd(cd, det), SINGLE + (lo.GRADS if det else ()))
    return c, cd, b, ref


@pytest.mark.parametrize("B,L", BWD_CASES)
def test_backward_stagewise(B, L):
    """One sample, one 16-sample chunk, one chunk + 1, two chunks + 5; a last pair of one position; a small odd L;
    five sample splits; workgroup 0 walking two pairs (with odd L and two chunks) and three pairs."""
    _backward_base(B, L, 0, _tag("bwd"))


@pytest.mark.parametrize("B,L", BWD_DET)
def test_backward_deterministic(B, L):
    """det = 1: one workgroup per pair walks every sample ((64, 80): five chunks), all six gradients repeat bitwise."""
    _backward_base(B, L, 1, _tag("bwd|det"))


@pytest.mark.parametrize("B,L", BWD_MODES)
def test_backward_launch_modes(B, L):
    """Against the reference of the slab form: dwl / dbl by atomics (no slab; a slab one row too small), fold = 0
    followed by the caller's pbx_colsum_add, and consts_ready = 1 with the first call's consts."""
    c, cd, base, ref = _backward_base(B, L, 0, _tag("bwd"))
    rows = _lib.lib().pbx_ln2_bwd_slab_rows(B, L, 0)
    for name, kw in (("atomic", dict(slab=None)), ("fallback", dict(slab="small")), ("fold0", dict(fold=0)),
                     ("ready", dict(consts=base["consts"]))):
        print(f"-- {name}")
        b = launch_bwd(cd, 0, **kw)
        if name == "fold0":
            for n in ("dwl", "dbl"):                          # nothing folded yet: the preloads, bit for bit
                assert torch.equal(b[n].v.view(torch.int32), cd[n + "_0"].view(torch.int32)), f"{n}: fold = 0 wrote it"
            sl = b["slab"].full
            _lib.call("pbx_colsum_add", sl.data_ptr(), rows, C * C, b["dwl"].full.data_ptr(), None, _st())
            _lib.call("pbx_colsum_add", sl.data_ptr() + rows * C * C * 4, rows, C, b["dbl"].full.data_ptr(), None, _st())
            torch.cuda.synchronize()
            _written(b, skip=("dgb",))
        _same_bits(base, b, SINGLE)
        lo.check_backward(c, _got_bwd(b, B, L), ref, LEDGER, None, _tag("bwd|" + name))


def test_backward_refusals():
    """det = 1 and fold = 0 need the slab: without one (or with one too small) the launcher refuses."""
    cd = _to_dev(lo.make_case(2, 33))
    for kw in (dict(det=1, slab=None), dict(det=1, slab="small"), dict(det=0, slab=None, fold=0),
               dict(det=0, slab="small", fold=0)):
        with pytest.raises(_lib.HipError, match="hipError 1$"):
            launch_bwd(cd, **kw)
        torch.cuda.synchronize()


@pytest.mark.parametrize("B,L,det", [(2, 33, 0), (17, 515, 0), (80, 64, 1)])
def test_backward_exact_library(B, L, det):
    with exact_library():
        _backward_base(B, L, det, _tag("bwd|det" if det else "bwd"))
    assert _lib.gelu_mode() != "custom"


# ---- embedding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1212, 3 * 512 + 1])
def test_embed_fwd(rows):
    """pbx_embed_fwd: bitwise the RNE bf16 of E[tok]; rows is no multiple of the 16-row block of a workgroup."""
    e = lo.make_embed_case(rows)
    ed = _to_dev(e)
    out = Buf(rows, C, dt=BF16)
    _lib.call("pbx_embed_fwd", ed["tok"].data_ptr(), ed["E"].data_ptr(), out.full.data_ptr(), rows, _st())
    torch.cuda.synchronize()
    out.assert_written("out")
    lo.check_embed_fwd(e, out.v.cpu())


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("rows", [1212, 3 * 512 + 1])
def test_embed_bwd(rows, slab):
    """pbx_embed_bwd, atomic and slab form: 1212 rows (3 workgroups of 404: two tiles each, the second partial) and
    3 x 512 + 1 (a fourth workgroup); V = 26 with every token present; dE preloaded."""
    e = lo.make_embed_case(rows)
    ed = _to_dev(e)
    groups = _lib.lib().pbx_embed_bwd_groups(rows)
    assert groups == (rows + 511) // 512

    def launch():
        b = dict(dE=Buf(V, C, fill=ed["dE0"]), slab=Buf(groups * V, C) if slab else None)
        _lib.call("pbx_embed_bwd", ed["tok"].data_ptr(), ed["dout"].data_ptr(), b["dE"].full.data_ptr(), rows, V,
                  None if not slab else b["slab"].full.data_ptr(), _st())
        torch.cuda.synchronize()
        _written(b)
        return b

    b = launch()
    lo.check_embed_bwd(e, b["dE"].v.cpu(), LEDGER, None, "embed_bwd|slab" if slab else "embed_bwd")
    if slab:
        _same_bits(b, launch(), ("dE",))
