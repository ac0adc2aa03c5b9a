"""Fine-tuning heads on the ProteinBERT encoder (BASELINE cfg 5).

The reference ships generic ``train_step``/``test_step`` loops (``ProteinBERT/utils.py:110-217``)
that call ``model(X)`` and apply ``loss_fn(logits, y)`` and ``softmax(logits, dim=1)``; it has no
fine-tuning model.  These heads follow that contract: the class axis is dim 1.

* :class:`ProteinBERTForTokenClassification` - per-residue head (e.g. 3- or 8-state secondary
  structure): logits ``[B, n_classes, L]``.
* :class:`ProteinBERTForSequenceClassification` - per-protein head on the global track:
  logits ``[B, n_classes]``.

``freeze_encoder=True`` runs the encoder under ``torch.no_grad`` (no activations are kept, so a
frozen-encoder step costs one forward of the fused HIP encoder plus the tiny head); with
``freeze_encoder=False`` gradients flow through the fused HIP backward as in pretraining.
Inputs: a token tensor ``[B, L]`` (annotations default to zeros, i.e. "no GO prior") or the
pretraining dict ``{"local": tokens, "global": annotations}``.

``hidden="last"`` (the default) reads the last block's output.  ``hidden="all"`` puts the task layer on the
concatenation of every block's hidden state, block 0 first: the local states ``h_i`` for the per-residue
head (``Linear(num_blocks * local_dim, K)``; on a GPU one streaming HIP launch over the ``num_blocks`` row
sources, :class:`..ops.finetune_head.MultiTokenHeadFn`), the global states ``g_i`` for the per-protein head
(``Linear(num_blocks * global_dim, n_classes)``; ``n_classes=1`` is the regression form, output ``[B, 1]``).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .proteinbert import ProteinBERT

Inputs = Union[torch.Tensor, Dict[str, torch.Tensor]]


def _split_inputs(model: ProteinBERT, x: Inputs) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(x, dict):
        return x["local"], x["global"]
    A = model.config["num_annotations"]
    return x, torch.zeros((x.shape[0], A), dtype=torch.float32, device=x.device)


HIDDEN = ("last", "all")


def encode(model: ProteinBERT, tokens: torch.Tensor, ann: torch.Tensor,
           tap: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Encoder output ``h [B, L, C]``, ``g [B, G]`` on the model's backend (fused HIP on a GPU).
    ``tap``: called as ``tap(i, h_i, g_i)`` after block ``i`` with that block's outputs."""
    if model.resolved_backend(tokens.device) == "hip":
        from ..ops.fused_model import fused_encode
        return fused_encode(model, tokens, ann.float(), tap=tap)
    return model.encode_torch(tokens, ann.float(), tap=tap)


class _FinetuneBase(nn.Module):
    def __init__(self, encoder: ProteinBERT, freeze_encoder: bool = True, hidden: str = "last"):
        super().__init__()
        if hidden not in HIDDEN:
            raise ValueError(f"hidden={hidden!r}: expected one of {HIDDEN}")
        self.encoder = encoder
        self.freeze_encoder = freeze_encoder
        self.hidden = hidden
        self.num_blocks = len(encoder.proteinBERT_blocks)
        if freeze_encoder:
            for p in encoder.parameters():
                p.requires_grad_(False)

    def _encode(self, x: Inputs) -> Tuple[torch.Tensor, torch.Tensor]:
        tokens, ann = _split_inputs(self.encoder, x)
        if self.freeze_encoder:
            with torch.no_grad():
                h, g = encode(self.encoder, tokens, ann)
            return h.detach(), g.detach()
        return encode(self.encoder, tokens, ann)

    def _encode_all(self, x: Inputs) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """Every block's ``(h_i, g_i)``, block 0 first.  The lists hold a reference to each block's output until
        the head has consumed it: both local tracks allocate a fresh output per block (``ops/local_track.py``
        ``h2``, ``ops/paper_track.py`` ``h2``; no buffer is recycled by a later block, with or without
        ``no_grad``), so a held reference is all that keeps the rows alive."""
        tokens, ann = _split_inputs(self.encoder, x)
        hs: List[torch.Tensor] = []
        gs: List[torch.Tensor] = []

        def tap(i, h_i, g_i):
            hs.append(h_i)
            gs.append(g_i)

        if self.freeze_encoder:
            with torch.no_grad():
                encode(self.encoder, tokens, ann, tap=tap)
            return [h.detach() for h in hs], [g.detach() for g in gs]
        encode(self.encoder, tokens, ann, tap=tap)
        return hs, gs

    def train(self, mode: bool = True):
        super().train(mode)
        if self.freeze_encoder:
            self.encoder.eval()
        return self


class ProteinBERTForTokenClassification(_FinetuneBase):
    def __init__(self, encoder: ProteinBERT, n_classes: int = 8, freeze_encoder: bool = True,
                 use_global: bool = True, dropout: float = 0.0, hidden: str = "last"):
        super().__init__(encoder, freeze_encoder, hidden)
        C, G = encoder.config["local_dim"], encoder.config["global_dim"]
        dev = encoder.local_embedding.weight.device
        self.use_global = use_global
        self.n_classes = n_classes
        self.dropout = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        nb = self.num_blocks if hidden == "all" else 1
        self.head = nn.Linear(nb * C, n_classes, device=dev)
        # per-residue logits = W_l h + (W_g g) broadcast over L  ==  Linear(concat(h, g))
        self.global_head = nn.Linear(nb * G, n_classes, bias=False, device=dev) if use_global else None

    def _forward_all(self, x: Inputs) -> torch.Tensor:
        hs, gs = self._encode_all(x)
        gterm = None
        if self.global_head is not None:
            gterm = self.global_head(torch.cat([g.float() for g in gs], dim=-1))          # [B, K]
        from ..ops import finetune_head
        if finetune_head.supported_multi(hs, self.n_classes) and isinstance(self.dropout, nn.Identity):
            # one streaming pass over the num_blocks row sources: the concatenation is never written
            logits = finetune_head.MultiTokenHeadFn.apply(*hs, self.head.weight, self.head.bias, gterm)
        else:
            feats = self.dropout(torch.cat([h.float() for h in hs], dim=-1))
            logits = F.linear(feats, self.head.weight, self.head.bias)                      # [B, L, K]
            if gterm is not None:
                logits = logits + gterm.unsqueeze(1)
        return logits.permute(0, 2, 1)                                                   # [B, K, L]

    def forward(self, x: Inputs) -> torch.Tensor:
        if self.hidden == "all":
            return self._forward_all(x)
        h, g = self._encode(x)
        from ..ops import finetune_head
        if finetune_head.supported(h, self.n_classes) and isinstance(self.dropout, nn.Identity):
            # fp32-accurate split-weight bf16 GEMMs on the encoder output + streaming weight-gradient
            # kernel (ops/finetune_head.py)
            logits = finetune_head.TokenHeadFn.apply(h, self.head.weight, self.head.bias)
        else:
            logits = F.linear(self.dropout(h.float()), self.head.weight, self.head.bias)    # [B, L, K]
        if self.global_head is not None:
            logits = logits + self.global_head(g.float()).unsqueeze(1)
        return logits.permute(0, 2, 1)                                                   # [B, K, L]

    def loss(self, x: Inputs, y: torch.Tensor, loss) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(loss, accuracy)`` of one training batch under ``loss``, a
        :class:`..train.task_loss.ResidueTaskLoss`: ``loss(self(x), y)`` and the accuracy of
        :func:`..train.finetune.token_accuracy` over the positions that are not ignored, both scalars on the
        device, from one encoder pass.  On a GPU (bf16 encoder rows, up to 16 classes, no dropout) the head, the
        loss, the accuracy and the gradient with respect to the logits are one HIP launch
        (:class:`..ops.finetune_head.TokenHeadLossFn`): the logits are never written.  There every negative label
        is ignored, so ``loss.ignore_index`` must be negative.  ``loss.counter(device)`` gains the batch's live
        positions, hits and labels ``>= n_classes``; such labels are kept out of the loss on either path."""
        from ..ops import finetune_head
        K = self.n_classes
        cw = loss.weights_on(y.device)
        if cw is not None and cw.numel() != K:
            raise ValueError(f"{cw.numel()} class weights for a head of {K} classes")
        counter = loss.counter(y.device)
        tokens = x["local"] if isinstance(x, dict) else x
        # decided before the encoder runs (its fused backend is what yields bf16 rows), so either path encodes once
        fusable = (finetune_head.LOSS_FUSED and isinstance(self.dropout, nn.Identity) and loss.ignore_index < 0
                   and y.dtype == torch.int64 and tokens.is_cuda and 1 <= K <= 16
                   and self.encoder.resolved_backend(tokens.device) == "hip")
        if fusable:
            if self.hidden == "all":
                hs, gs = self._encode_all(x)
                gin = torch.cat([g.float() for g in gs], dim=-1) if self.global_head is not None else None
            else:
                h, g = self._encode(x)
                hs, gin = [h], (g.float() if self.global_head is not None else None)
            if finetune_head.supported_loss(hs, K) and y.device == hs[0].device:
                gterm = None if gin is None else self.global_head(gin)                          # [B, K]
                return finetune_head.TokenHeadLossFn.apply(*hs, self.head.weight, self.head.bias, gterm, y, cw,
                                                           loss.label_smoothing, counter)
            del hs
        logits = self.forward(x)
        bad = y >= K
        yc = torch.where(bad, torch.full_like(y, loss.ignore_index), y)
        value = loss(logits, yc)
        with torch.no_grad():
            valid = yc != loss.ignore_index
            hits = ((torch.softmax(logits.detach().float(), dim=1).argmax(1) == yc) & valid).sum()
            n_valid = valid.sum()
            counter += torch.stack([n_valid, hits, bad.sum()])
            acc = hits.float() / n_valid.clamp_min(1).float()
        return value, acc


class ProteinBERTForSequenceClassification(_FinetuneBase):
    def __init__(self, encoder: ProteinBERT, n_classes: int = 2, freeze_encoder: bool = True,
                 dropout: float = 0.0, hidden: str = "last"):
        super().__init__(encoder, freeze_encoder, hidden)
        G = encoder.config["global_dim"]
        dev = encoder.local_embedding.weight.device
        self.n_classes = n_classes
        self.dropout = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.head = nn.Linear((self.num_blocks if hidden == "all" else 1) * G, n_classes, device=dev)

    def forward(self, x: Inputs) -> torch.Tensor:
        if self.hidden == "all":
            _, gs = self._encode_all(x)
            return self.head(self.dropout(torch.cat([g.float() for g in gs], dim=-1)))
        _, g = self._encode(x)
        return self.head(self.dropout(g.float()))


def build_finetune_model(enc: ProteinBERT, meta: dict, freeze_encoder: bool = True):
    """The head class a saved head file's ``meta`` describes (:func:`load_finetuned_head`)."""
    if meta["task"] == "residue":
        return ProteinBERTForTokenClassification(enc, n_classes=meta["n_classes"], freeze_encoder=freeze_encoder,
                                                 use_global=meta["use_global"], hidden=meta["hidden"])
    return ProteinBERTForSequenceClassification(enc, n_classes=meta["n_classes"], freeze_encoder=freeze_encoder,
                                                hidden=meta["hidden"])


def load_finetuned_head(path: str, enc: ProteinBERT, freeze_encoder: bool = True):
    """Rebuild the fine-tuned model of a ``proteinbert_finetuned_head.pt`` around ``enc``.  The file's ``"meta"``
    entry names the task and head form; a file without it is a ``hidden="last"`` per-residue head."""
    state = dict(torch.load(path, map_location="cpu"))
    meta = state.pop("meta", None)
    if meta is None:
        meta = {"task": "residue", "hidden": "last", "n_classes": state["head.weight"].shape[0], "classes": None,
                "use_global": "global_head.weight" in state}
    model = build_finetune_model(enc, meta, freeze_encoder)
    missing, unexpected = model.load_state_dict(state, strict=False)
    if unexpected or any(not k.startswith("encoder.") for k in missing):
        raise ValueError(f"{path}: head does not fit meta {meta}: missing "
                         f"{[k for k in missing if not k.startswith('encoder.')]}, unexpected {unexpected}")
    return model, meta
