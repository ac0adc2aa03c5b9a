"""Per-residue fine-tuning head on MI355X (BASELINE cfg 5).

``logits = h Wᵀ + b`` over ``[B*L, 128]`` bf16 encoder rows and K <= 16 classes.  The head weight
stays an fp32 parameter and the logits keep fp32 accuracy: one streaming kernel (``csrc/finetune.hip``
``token_head_fwd``, a thread per residue, W broadcast from LDS) runs fp32 FMAs over the exact bf16
rows -- the fp32 ``F.linear`` result on an upcast copy, memory-bound on the 67 MB row read at
B*L = 262,144 (round 3-4 used two library bf16 GEMMs on a hi / lo weight split, 2 x 25 us).  The weight gradient, a 262,144-long reduction that hipBLASLt ran at 230-410 us,
is the streaming kernel in ``csrc/finetune.hip`` (fp32 accumulation, deterministic slab reduction);
the input gradient (unfrozen encoders only) is fp32.

``hidden="all"`` heads read every block's hidden state: :class:`MultiTokenHeadFn` is the same pair of
kernels over up to 8 row sources (``token_head_multi_fwd`` / ``token_head_multi_wgrad``), so the
concatenated ``[B*L, nb*128]`` feature matrix (and its fp32 copy) is never written.

Training on a shaped loss: :class:`TokenHeadLossFn` is one launch (``token_head_loss``) that keeps the logits
in registers and writes the gradient of the class-weighted, label-smoothed cross-entropy with respect to them,
plus per-workgroup loss / weight / accuracy partials that ``token_head_loss_fold`` turns into the step's loss,
its ``1 / sum w`` and the accuracy on the device.  The backward feeds that gradient to the same weight-gradient
kernels; the fp32 logits, their permute, the loss ops and the softmax / argmax of the metric never run.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib

MAX_SOURCES = 8


def supported(h: torch.Tensor, n_classes: int) -> bool:
    return h.is_cuda and h.dtype == torch.bfloat16 and h.shape[-1] == 128 and n_classes <= 16


class TokenHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias):
        B, L, C = h.shape
        h2 = h.contiguous().view(B * L, C)
        K = weight.shape[0]
        # one streaming pass: fp32 FMAs over the exact bf16 rows and fp32 weights (csrc/finetune.hip)
        logits = torch.empty((B * L, K), dtype=torch.float32, device=h.device)
        _lib.call("pbx_token_head_fwd", h2.data_ptr(), weight.detach().float().contiguous().data_ptr(),
                  bias.detach().float().contiguous().data_ptr(), logits.data_ptr(), B * L, K,
                  _lib.stream_ptr(h.device))
        ctx.save_for_backward(h2, weight)
        ctx.shape = (B, L)
        return logits.view(B, L, -1)

    @staticmethod
    def backward(ctx, dlogits):
        h2, weight = ctx.saved_tensors
        B, L = ctx.shape
        K = weight.shape[0]
        g = dlogits.reshape(B * L, K).float().contiguous()
        dh = dw = db = None
        if ctx.needs_input_grad[0]:
            dh = torch.mm(g, weight.float()).view(B, L, -1).to(h2.dtype)
        if ctx.needs_input_grad[1]:
            M = B * L
            P = max(1, min(2 * torch.cuda.get_device_properties(h2.device).multi_processor_count, (M + 15) // 16))
            slab = torch.empty((P, K, h2.shape[1]), dtype=torch.float32, device=h2.device)
            st = _lib.stream_ptr(h2.device)
            _lib.call("pbx_token_head_wgrad", h2.data_ptr(), g.data_ptr(), slab.data_ptr(), M, K, P, st)
            dw = torch.zeros_like(weight)
            _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * h2.shape[1], dw.data_ptr(), None, st)
        if ctx.needs_input_grad[2]:
            db = g.sum(dim=0)
        return dh, dw, db


def supported_multi(hs: Sequence[torch.Tensor], n_classes: int) -> bool:
    """The fused all-block head: 1..8 CUDA bf16 ``[B, L, 128]`` sources of one shape and K <= 16."""
    if not 1 <= len(hs) <= MAX_SOURCES or not 1 <= n_classes <= 16:
        return False
    h0 = hs[0]
    return all(h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and h.shape[-1] == 128
               and h.shape == h0.shape and h.device == h0.device for h in hs)


def multi_head_torch(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                     gterm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition on any device: ``Linear(cat_i h_i) + gterm`` broadcast over L, in fp32."""
    logits = torch.nn.functional.linear(torch.cat([h.float() for h in hs], dim=-1), weight, bias)
    return logits if gterm is None else logits + gterm.unsqueeze(1)


def _rows(h: torch.Tensor) -> torch.Tensor:
    """``[B, L, 128]`` as row-contiguous, 16-byte aligned ``[B*L, 128]`` (a copy only when it is not already)."""
    h2 = h.contiguous().view(-1, h.shape[-1])
    return h2 if h2.data_ptr() % 16 == 0 else h2.clone()


def _src_array(rows: List[torch.Tensor]):
    """Host array of the sources' device addresses (the launcher copies it into the kernel's arguments)."""
    return (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])


def wgrad_slab_rows(M: int, device) -> int:
    return max(1, min(2 * torch.cuda.get_device_properties(device).multi_processor_count, (M + 15) // 16))


class MultiTokenHeadFn(torch.autograd.Function):
    """``apply(h_0, ..., h_{nb-1}, weight [K, nb*128], bias [K], gterm [B, K] | None)`` -> logits ``[B, L, K]``:
    ``bias + sum_i h_i @ weight[:, i*128:(i+1)*128].T + gterm`` broadcast over L, fp32 FMAs over the exact bf16
    rows, blocks in ascending order."""

    @staticmethod
    def forward(ctx, *args):
        hs, (weight, bias, gterm) = args[:-3], args[-3:]
        nb = len(hs)
        B, L, C = hs[0].shape
        K = weight.shape[0]
        if weight.shape[1] != nb * C:
            raise ValueError(f"weight {tuple(weight.shape)} for {nb} sources of {C} channels")
        M = B * L
        rows = [_rows(h) for h in hs]
        gt = None if gterm is None else gterm.detach().float().contiguous()
        if gt is not None and tuple(gt.shape) != (B, K):
            raise ValueError(f"gterm {tuple(gt.shape)}: expected {(B, K)}")
        w32 = weight.detach().float().contiguous()
        b32 = bias.detach().float().contiguous()
        logits = torch.empty((M, K), dtype=torch.float32, device=hs[0].device)
        _lib.call("pbx_token_head_multi_fwd", _src_array(rows), nb, w32.data_ptr(), b32.data_ptr(), _lib.ptr(gt),
                  logits.data_ptr(), M, K, L, _lib.stream_ptr(hs[0].device))
        ctx.save_for_backward(weight, *rows)
        ctx.shape = (B, L, nb)
        ctx.has_gterm = gterm is not None
        return logits.view(B, L, K)

    @staticmethod
    def backward(ctx, dlogits):
        weight, *rows = ctx.saved_tensors
        B, L, nb = ctx.shape
        K, C = weight.shape[0], rows[0].shape[1]
        M = B * L
        g = dlogits.reshape(M, K).float().contiguous()
        dhs = [None] * nb
        if any(ctx.needs_input_grad[:nb]):
            w32 = weight.float()
            for i in range(nb):
                if ctx.needs_input_grad[i]:
                    dhs[i] = torch.mm(g, w32[:, i * C:(i + 1) * C]).view(B, L, C).to(rows[i].dtype)
        dw = db = dgt = None
        if ctx.needs_input_grad[nb]:
            dev = rows[0].device
            P = wgrad_slab_rows(M, dev)
            slab = torch.empty((P, K, nb * C), dtype=torch.float32, device=dev)
            st = _lib.stream_ptr(dev)
            _lib.call("pbx_token_head_multi_wgrad", _src_array(rows), nb, g.data_ptr(), slab.data_ptr(), M, K, P, st)
            dw = torch.zeros_like(weight)
            _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * nb * C, dw.data_ptr(), None, st)
        if ctx.needs_input_grad[nb + 1]:
            db = g.sum(dim=0)
        if ctx.has_gterm and ctx.needs_input_grad[nb + 2]:
            dgt = g.view(B, L, K).sum(dim=1)
        return (*dhs, dw, db, dgt)


# ---- the training loss of a per-residue head, fused ---------------------------------------------------------
LOSS_FUSED = True        # False: ProteinBERTForTokenClassification.loss takes the torch form on every device


def supported_loss(hs: Sequence[torch.Tensor], n_classes: int) -> bool:
    """The fused training loss: the sources and class counts of :func:`supported_multi`."""
    return supported_multi(hs, n_classes)


def loss_parts(M: int) -> int:
    """Workgroups (= partial rows) of ``pbx_token_head_loss`` on ``M`` rows: ``(M + 255) // 256``."""
    return int(_lib.lib().pbx_token_head_loss_parts(int(M)))


def token_head_loss_torch(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                          gterm: Optional[torch.Tensor], y: torch.Tensor, cw: Optional[torch.Tensor] = None,
                          eps: float = 0.0, ignore_index: int = -100) -> Tuple[torch.Tensor, torch.Tensor]:
    """The definition on any device: ``(loss, accuracy)`` = ``F.cross_entropy(z, y, weight=cw,
    label_smoothing=eps)`` over the logits ``z`` of :func:`multi_head_torch` (rows whose label is negative are
    ignored, whatever ``ignore_index`` names among them), and the share of live rows whose first maximal class
    is the label."""
    z = multi_head_torch(hs, weight, bias, gterm)
    K = z.shape[-1]
    z2, yf = z.reshape(-1, K), y.reshape(-1)
    live = yf >= 0
    yt = torch.where(live, yf, torch.full_like(yf, ignore_index))
    loss = F.cross_entropy(z2, yt, weight=cw, ignore_index=ignore_index, label_smoothing=float(eps))
    with torch.no_grad():
        hit = (torch.softmax(z2.detach().float(), -1).argmax(-1) == yf) & live
        acc = hit.sum().float() / live.sum().clamp_min(1).float()
    return loss, acc


class TokenHeadLossFn(torch.autograd.Function):
    """``apply(h_0, ..., h_{nb-1}, weight [K, nb*128], bias [K], gterm [B, K] | None, y [B, L] int64,
    cw [K] | None, eps, acc_cnt [3] int64)`` -> ``(loss, accuracy)``, two device scalars, no host sync.

    ``loss`` is ``F.cross_entropy(logits, y, weight=cw, label_smoothing=eps)`` with ``y < 0`` ignored;
    ``accuracy`` the share of live rows called as their label (not differentiable).  ``acc_cnt`` gains (live rows,
    hits, labels >= K): the caller reads it when it next syncs and treats a non-zero third entry as an error.
    The backward scales the reduced gradients by ``grad_out / sum w`` and never makes another pass over the
    ``[B*L, K]`` logit gradient."""

    @staticmethod
    def forward(ctx, *args):
        hs, (weight, bias, gterm, y, cw, eps, acc_cnt) = args[:-7], args[-7:]
        nb = len(hs)
        B, L, C = hs[0].shape
        K = weight.shape[0]
        eps = float(eps)
        if weight.shape[1] != nb * C:
            raise ValueError(f"weight {tuple(weight.shape)} for {nb} sources of {C} channels")
        if not 0.0 <= eps < 1.0:
            raise ValueError(f"label smoothing {eps}: expected 0 <= eps < 1")
        if tuple(y.shape) != (B, L) or y.dtype != torch.int64 or y.device != hs[0].device:
            raise ValueError(f"y must be int64 {(B, L)} on {hs[0].device}")
        if cw is not None and tuple(cw.shape) != (K,):
            raise ValueError(f"class weights {tuple(cw.shape)}: expected {(K,)}")
        if tuple(acc_cnt.shape) != (3,) or acc_cnt.dtype != torch.int64 or acc_cnt.device != hs[0].device:
            raise ValueError("acc_cnt must be int64 [3] on the sources' device")
        gt = None if gterm is None else gterm.detach().float().contiguous()
        if gt is not None and tuple(gt.shape) != (B, K):
            raise ValueError(f"gterm {tuple(gt.shape)}: expected {(B, K)}")
        M = B * L
        dev = hs[0].device
        rows = [_rows(h) for h in hs]
        w32 = weight.detach().float().contiguous()
        b32 = bias.detach().float().contiguous()
        cw32 = None if cw is None else cw.detach().to(dev, torch.float32).contiguous()
        yc = y.contiguous()
        nwg = loss_parts(M)
        g = torch.empty((M, K), dtype=torch.float32, device=dev)
        part = torch.empty((nwg, 2), dtype=torch.float32, device=dev)
        cnt = torch.empty((nwg, 3), dtype=torch.int32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        st = _lib.stream_ptr(dev)
        _lib.call("pbx_token_head_loss", _src_array(rows), nb, w32.data_ptr(), b32.data_ptr(), _lib.ptr(gt),
                  yc.data_ptr(), _lib.ptr(cw32), eps, g.data_ptr(), part.data_ptr(), cnt.data_ptr(), M, K, L, st)
        _lib.call("pbx_token_head_loss_fold", part.data_ptr(), cnt.data_ptr(), nwg, out.data_ptr(),
                  acc_cnt.data_ptr(), st)
        ctx.save_for_backward(weight, g, out, *rows)
        ctx.shape = (B, L, nb)
        ctx.has_gterm = gterm is not None
        loss, acc = out[0].clone(), out[2].clone()
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, dloss, _dacc):
        weight, g, out, *rows = ctx.saved_tensors
        B, L, nb = ctx.shape
        K, C = weight.shape[0], rows[0].shape[1]
        M = B * L
        s = dloss.float() * out[1]                                  # one element, on the device
        dhs = [None] * nb
        if any(ctx.needs_input_grad[:nb]):
            w32 = weight.float()
            for i in range(nb):
                if ctx.needs_input_grad[i]:
                    dhs[i] = (torch.mm(g, w32[:, i * C:(i + 1) * C]) * s).view(B, L, C).to(rows[i].dtype)
        dw = db = dgt = None
        if ctx.needs_input_grad[nb]:
            dev = rows[0].device
            P = wgrad_slab_rows(M, dev)
            slab = torch.empty((P, K, nb * C), dtype=torch.float32, device=dev)
            st = _lib.stream_ptr(dev)
            if nb == 1:
                _lib.call("pbx_token_head_wgrad", rows[0].data_ptr(), g.data_ptr(), slab.data_ptr(), M, K, P, st)
            else:
                _lib.call("pbx_token_head_multi_wgrad", _src_array(rows), nb, g.data_ptr(), slab.data_ptr(), M, K,
                          P, st)
            dw = torch.zeros(weight.shape, dtype=torch.float32, device=dev)
            _lib.call("pbx_colsum_add", slab.data_ptr(), P, K * nb * C, dw.data_ptr(), None, st)
            dw = (dw * s).to(weight.dtype)
        if ctx.needs_input_grad[nb + 1]:
            db = g.sum(dim=0) * s
        if ctx.has_gterm and ctx.needs_input_grad[nb + 2]:
            dgt = g.view(B, L, K).sum(dim=1) * s
        return (*dhs, dw, db, dgt, None, None, None, None)
