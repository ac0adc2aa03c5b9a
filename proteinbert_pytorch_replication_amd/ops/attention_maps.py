"""Attention maps: the weights of the paper-semantics global attention, per block and head (``csrc/attn_maps.hip``).

The global attention of ``semantics="paper"`` (one query per head from the global track, a softmax over the
positions of the local track) is the interpretable part of ProteinBERT.  The encoder never stores its weights:
``pa_fused_fwd_kernel`` keeps them in LDS for one tile.  Here they are computed from the states the encoder's taps
hand out (``fused_encode(..., tap=, tap_input=)``).  For block ``i`` with ``h2_i [B, L, 128]`` (the block's local
output), ``g_in_i [B, G]`` (the global vector that ENTERS the block: the input layer's output for block 0, else
the previous block's ``g``) and ``mask = tokens != <pad>``::

    qs[b,h,:]  = tanh(g_in[b] Wq[h]) / sqrt(K)               fp32
    a[b,h,l,:] = h2[b,l,:] . Wk[h]                           bf16 x bf16(Wk), fp32 accumulation (HIP)
    s[b,h,l]   = sum_k qs[b,h,k] * tanh(a[b,h,l,k])
    p[b,h,:]   = softmax of s over the positions with mask; exactly 0.0 at <pad>; no live position: all zeros

``<sos>`` and ``<eos>`` are positions the model attends to and are not masked.

* :func:`attention_maps` -- the HIP path: ``pbx_sg_query_fwd`` (``qs``) and ``pbx_pa_wimg`` (the bf16 key rows)
  per block, then ``pbx_attn_map_scores`` + ``pbx_attn_map_normalize`` once per group of up to 8 blocks, writing
  ``[B, blocks, H, L]`` fp32 directly.  No atomics; a row's bits depend on that row's states, the weights and
  ``L`` only (not on the batch, the row's place in it, the blocks in the launch or the grid).
* :func:`attention_maps_torch` -- the same definition in fp32 on any device: the CPU, the torch backend,
  deterministic mode and the shapes outside :func:`attention_supported`.

In reference semantics the softmax runs over K identical query rows: every weight is ``1/K`` by construction and
``Wq`` / ``Wk`` never influence the model, so there is no attention map to show (:mod:`..inference` refuses).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ..data.vocab import PAD_ID

F32 = torch.float32
KEY_DIM = 64
LOCAL_DIM = 128
MAX_HEADS = 8                   # pbx_attn_map_scores: every head's 16 KB key image in LDS at once
MAX_BLOCKS = 8                  # ... and at most 8 blocks per launch (more: several launches)
CHUNK = 256                     # positions per (max, sum exp) partial


def _shapes(h2s: Sequence[torch.Tensor], g_ins: Sequence[torch.Tensor], Wqs: Sequence[torch.Tensor],
            Wks: Sequence[torch.Tensor], tokens: Optional[torch.Tensor]) -> Tuple[int, int, int, int]:
    """``(B, L, H, blocks)`` of a call, or ``ValueError``: shapes only, so it holds on any device."""
    nb = len(h2s)
    if nb < 1 or not (len(g_ins) == len(Wqs) == len(Wks) == nb):
        raise ValueError(f"attention_maps: {nb} local states, {len(g_ins)} global inputs, {len(Wqs)} Wq and "
                         f"{len(Wks)} Wk: expected one of each per block, at least one block")
    h0 = h2s[0]
    if h0.dim() != 3 or h0.shape[0] < 1 or h0.shape[1] < 1:
        raise ValueError(f"attention_maps: h2 {tuple(h0.shape)}: expected a non-empty [B, L, C] tensor")
    B, L, C = h0.shape
    if Wks[0].dim() != 3:
        raise ValueError(f"attention_maps: Wk {tuple(Wks[0].shape)}: expected [H, C, K]")
    H, _, K = Wks[0].shape
    for i in range(nb):
        if h2s[i].shape != h0.shape or h2s[i].dtype != h0.dtype or h2s[i].device != h0.device:
            raise ValueError("attention_maps: the local states must be [B, L, C] tensors of one shape, dtype and "
                             "device")
        if g_ins[i].dim() != 2 or g_ins[i].shape[0] != B:
            raise ValueError(f"attention_maps: g_in {tuple(g_ins[i].shape)}: expected [{B}, G]")
        if tuple(Wks[i].shape) != (H, C, K):
            raise ValueError(f"attention_maps: Wk {tuple(Wks[i].shape)}: expected {(H, C, K)}")
        if tuple(Wqs[i].shape) != (H, g_ins[i].shape[1], K):
            raise ValueError(f"attention_maps: Wq {tuple(Wqs[i].shape)}: expected {(H, g_ins[i].shape[1], K)}")
    if tokens is not None and tuple(tokens.shape) != (B, L):
        raise ValueError(f"attention_maps: tokens {tuple(tokens.shape)}: expected {(B, L)}")
    return B, L, H, nb


def attention_supported(h2s: Sequence[torch.Tensor], Wks: Sequence[torch.Tensor]) -> bool:
    """Whether :func:`attention_maps` takes these states: CUDA bf16 ``[B, L, 128]``, ``key_dim = 64`` and at most
    8 heads (any number of blocks: more than 8 take several launches).  Outside:
    :func:`attention_maps_torch`."""
    if len(h2s) < 1 or len(Wks) != len(h2s) or Wks[0].dim() != 3:
        return False
    H, C, K = Wks[0].shape
    return (all(h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and h.shape[-1] == LOCAL_DIM for h in h2s)
            and C == LOCAL_DIM and K == KEY_DIM and 1 <= H <= MAX_HEADS)


def grid_cap(H: int) -> int:
    """The most workgroups a ``pbx_attn_map_scores`` launch of ``H`` heads uses (CUs x workgroups per CU); with
    more (block, sample, chunk) items its workgroups walk several."""
    return int(_lib.lib().pbx_attn_map_grid_cap(int(H)))


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _addr_array(ts: Sequence[torch.Tensor]):
    """Host array of device addresses (the launcher copies it into the kernel's arguments)."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def attention_maps(h2s: Sequence[torch.Tensor], g_ins: Sequence[torch.Tensor], Wqs: Sequence[torch.Tensor],
                   Wks: Sequence[torch.Tensor], tokens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The attention weights ``[B, blocks, H, L]`` fp32 of every block and head (the module docstring's
    definition) on the HIP path: ``h2s[i] [B, L, 128]`` bf16, ``g_ins[i] [B, G]``, ``Wqs[i] [H, G, 64]``,
    ``Wks[i] [H, 128, 64]``, ``tokens [B, L]`` (``<pad>`` positions get weight 0; None: no mask).  Raises
    ``ValueError`` outside :func:`attention_supported`, before any launch."""
    B, L, H, nb = _shapes(h2s, g_ins, Wqs, Wks, tokens)
    if not attention_supported(h2s, Wks):
        raise ValueError("attention_maps: the local states must be CUDA bf16 [B, L, 128] tensors, key_dim 64 and "
                         f"at most {MAX_HEADS} heads (attention_maps_torch is the definition on any device)")
    dev = h2s[0].device
    if tokens is not None and tokens.device != dev:
        raise ValueError("attention_maps: tokens must be on the states' device")
    st = _lib.stream_ptr(dev)
    mask = None if tokens is None else (tokens != PAD_ID).contiguous()
    rows = [_aligned(h) for h in h2s]
    # per block: qs = tanh(g Wq) / sqrt(K) in fp32 and the bf16 key rows [H][64][128], as the encoder forms them;
    # one split-K workspace and one q scratch serve every block (stream order)
    G = max(g.shape[1] for g in g_ins)
    ws = torch.empty(_lib.lib().pbx_sg_query_ws(B, G, H, KEY_DIM), dtype=F32, device=dev)
    q = torch.empty((B, H, KEY_DIM), dtype=F32, device=dev)
    qss = torch.empty((nb, B, H, KEY_DIM), dtype=F32, device=dev)
    wimg = torch.empty((nb, H, KEY_DIM, LOCAL_DIM), dtype=torch.bfloat16, device=dev)
    for i in range(nb):
        gf = g_ins[i].detach().float().contiguous()
        wq32 = Wqs[i].detach().float().contiguous()
        wk32 = Wks[i].detach().float().contiguous()
        _lib.call("pbx_sg_query_fwd", gf.data_ptr(), wq32.data_ptr(), q.data_ptr(), qss[i].data_ptr(), ws.data_ptr(),
                  B, gf.shape[1], H, KEY_DIM, 1.0 / math.sqrt(KEY_DIM), st)
        _lib.call("pbx_pa_wimg", wk32.data_ptr(), wk32.data_ptr(), wimg[i].data_ptr(), H, LOCAL_DIM, KEY_DIM, 0, st)
    out = torch.empty((B, nb, H, L), dtype=F32, device=dev)
    part = torch.empty((B * nb * H, -(-L // CHUNK), 2), dtype=F32, device=dev)
    for b0 in range(0, nb, MAX_BLOCKS):
        n = min(MAX_BLOCKS, nb - b0)
        _lib.call("pbx_attn_map_scores", _addr_array(rows[b0:b0 + n]), _addr_array([wimg[b0 + i] for i in range(n)]),
                  _addr_array([qss[b0 + i] for i in range(n)]), _lib.ptr(mask), out.data_ptr(), part.data_ptr(),
                  B, L, H, n, b0, nb, st)
        _lib.call("pbx_attn_map_normalize", out.data_ptr(), part.data_ptr(), B, L, H, n, b0, nb, st)
    return out


def attention_maps_torch(h2s: Sequence[torch.Tensor], g_ins: Sequence[torch.Tensor], Wqs: Sequence[torch.Tensor],
                         Wks: Sequence[torch.Tensor], tokens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`attention_maps` by definition, in fp32 on any device and for any dimensions: ``[B, blocks, H, L]``.
    Each row is computed from that row alone."""
    B, L, H, nb = _shapes(h2s, g_ins, Wqs, Wks, tokens)
    dev = h2s[0].device
    mask = None if tokens is None else (tokens.to(dev) != PAD_ID)
    maps = []
    for h2, g, Wq, Wk in zip(h2s, g_ins, Wqs, Wks):
        K = Wk.shape[2]
        qs = torch.tanh(torch.einsum("bg,hgk->bhk", g.detach().float(), Wq.detach().float())) / math.sqrt(K)
        a = torch.einsum("blc,hck->bhlk", h2.detach().float(), Wk.detach().float())
        s = torch.einsum("bhk,bhlk->bhl", qs, torch.tanh(a))
        if mask is not None:
            s = s.masked_fill(~mask.unsqueeze(1), float("-inf"))
            # a row without a live position: zeros (its softmax is 0 / 0)
            p = torch.where(mask.any(dim=1)[:, None, None], torch.softmax(s, dim=-1), torch.zeros_like(s))
        else:
            p = torch.softmax(s, dim=-1)
        maps.append(p)
    return torch.stack(maps, dim=1)
