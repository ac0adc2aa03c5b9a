"""Using a pretrained ProteinBERT as a model: embeddings, GO-term predictions and residue calls.

:class:`Predictor` wraps a :class:`~.models.ProteinBERT` and answers, for a list of protein sequences (or
token tensors), any subset of

===================  ==========================================================  =======================
``outputs`` name     entries of the result                                       dtype
===================  ==========================================================  =======================
``global``           ``global`` ``[N, G]``: the global track's final vector      fp32
``pooled``           ``pooled`` ``[N, 128]``: mean of the local track over the   fp32
                     non-``<pad>`` positions
``residue``          ``residue`` ``[N, L, 128]``: the local track                bf16 (HIP) / fp32
``go_probs``         ``go_probs`` ``[N, A]``                                     fp32
``go_topk``          ``go_topk_values`` / ``go_topk_indices`` ``[N, k]``         fp32 / int32
``residue_probs``    ``residue_probs`` ``[N, L, V]``                             fp32
``residue_tokens``   ``residue_tokens`` / ``residue_token_probs`` ``[N, L]``     int32 / fp32
``hidden_states``    ``hidden_global`` ``[N, blocks, G]`` / ``hidden_pooled``    fp32
                     ``[N, blocks, 128]``: ``global`` / ``pooled`` after every
                     block
``residue_llr``      ``residue_llr`` ``[N, L, V]``: log-odds of substituting     fp32
                     every token at every position
``residue_logp``     ``residue_logp`` ``[N, L]``: log-probability of the         fp32
                     residue that is there
``residue_entropy``  ``residue_entropy`` ``[N, L]``: entropy over the            fp32
                     vocabulary, in nats
``pll``              ``pll`` ``[N]``: pseudo-log-likelihood; ``n_residues``      fp32 / int32
                     ``[N]``: the positions it sums over
``attention``        ``attention`` ``[N, blocks, H, L]``: the weights of the     fp32
                     global attention, per block and head (paper semantics
                     only)
``attention_top``    ``attention_top_values`` / ``attention_top_indices``        fp32 / int32
                     ``[N, blocks, H, k]``: the ``k`` most attended positions
                     per block and head (paper semantics only)
``task:NAME``        ``task_NAME_labels`` / ``task_NAME_label_probs``:           int32 / fp32
                     ``[N, L]`` (residue head) or ``[N]`` (per-protein
                     classifier); a regression head (``n_classes == 1``) gives
                     ``task_NAME_values`` ``[N]`` (fp32) instead
``task_probs:NAME``  ``task_NAME_probs``: ``[N, L, K]`` (residue head) or        fp32
                     ``[N, n]`` (per-protein classifier); a regression head
                     raises ``ValueError``
===================  ==========================================================  =======================

``task:NAME`` / ``task_probs:NAME`` exist for the fine-tuned heads registered as ``Predictor(model,
heads={NAME: head})`` (:mod:`.models.finetune`; a head instance around ``model``, or the path of a file written
by ``cli finetune``); any other name raises ``unknown outputs``.  Only the head's own layers are used (``head``,
``global_head``), on the batch's single encoder pass, whatever the number of heads.  A residue head's call is the
lowest class of maximal probability; at the positions fine-tuning ignores (``<pad>``, ``<sos>``, ``<eos>``: token
id below ``UNK_ID``, the ones ``cli finetune`` labels -100) the label is -1, the probability 0 and the
probability row zero.  On the HIP backend a residue head is one launch of ``pbx_token_head_calls``
(:func:`.ops.infer_heads.token_head_calls`) whose logits never leave the registers; its global term
(``global_head`` of ``g``, or of the concatenated per-block ``g_i``) is a ``[B, K]`` torch op.  The per-protein
heads are ``[B, n]``-sized torch ops on both backends: a few KB per batch, where a kernel would gain nothing.

Only the requested heads run.  On the HIP backend (``model.resolved_backend(device) == "hip"``) the encoder is
:func:`.ops.fused_model.fused_encode` and the heads are the fused kernels of :mod:`.ops.infer_heads`; on the
PyTorch backend the same outputs come from ``encode_torch`` + ``heads_torch`` with the same tie rules (GO
top-k: descending, equal probabilities by ascending index, a stable sort; residue call: the first maximal
index; pooling: a masked mean in fp32).

**Reference semantics: local predictions depend on batch mates.**  The reference's local head normalises
every (position, token) over the BATCH axis (``modules.py:277-284``), so ``residue_probs`` /
``residue_tokens`` / ``residue_token_probs`` of a sequence change with the sequences it shares a batch with,
and a batch of one gives probabilities of exactly 1 everywhere.  That is the reference's behaviour and is not
corrected here: :meth:`Predictor.predict` normalises over each of its batches of ``batch_size`` sequences (the
last one may be smaller), on this process only.  Keep ``batch_size`` and the input order fixed to compare
runs, or use a ``semantics="paper"`` model (softmax over the vocabulary), whose predictions are per sequence.
Embeddings and GO predictions do not depend on the batch in either semantics.  Neither do the ``task:`` /
``task_probs:`` outputs: a task head's softmax runs over its classes, per residue or per protein, so they are
per sequence whatever the model's semantics (the encoder itself never mixes sequences).

**Scores: variant effects and pseudo-log-likelihood.**  ProteinBERT is a denoising model without a mask token,
so a sequence is scored by the wild-type marginal: one encoder pass over the unmodified sequence, then
arithmetic on the local head's logits ``z[p, v]``.  With ``x`` the token at a position and the position *live*
when ``UNK_ID <= x < V`` (the task heads' rule: not ``<pad>``, ``<sos>``, ``<eos>``; an id outside the
vocabulary is not live either): ``residue_llr[p, a] = z[a] - z[x]`` (a difference of logits, the column of
``x`` exactly ``+0.0``), ``residue_logp[p] = log softmax_v(z)[x]``, ``residue_entropy[p]`` the entropy of
``softmax_v(z)`` in nats; zeros where the position is not live.  ``pll`` is the sum of ``residue_logp`` over the
``n_residues`` live positions (fp64 accumulation in a fixed order, rounded once; 0 for a sequence without one);
the pseudo-perplexity ``exp(-pll / n_residues)`` is left to the caller and is ``nan`` for such a sequence.  On
the HIP backend these are ``pbx_lhead_scores`` + ``pbx_seq_score_fold`` (:func:`.ops.infer_heads.local_scores`;
the ``[N, L, V]`` matrix is written only when ``residue_llr`` is requested), on the PyTorch backend
:func:`.ops.infer_heads.local_scores_torch`.  They are computed from the logits, which are per row in both
semantics, so they do not depend on batch mates.  For a paper-semantics model ``residue_logp`` is the log of
the model's own ``residue_probs`` at the wild-type token.  For a reference-semantics model these quantities are
functions of the logits under a vocabulary softmax: that is NOT the batch-axis quantity the model was trained
on.  :meth:`Predictor.score_variants` and :meth:`Predictor.mutation_scan` are built on these outputs.

**Attention maps: where the model looks.**  The global attention of a ``semantics="paper"`` model (one query per
head from the global track, a softmax over the positions of the local track) is the interpretable part of the
architecture.  For block ``i`` with its local output ``h2_i``, the global vector ``g_in_i`` that enters it (the
input layer's output for block 0, else the previous block's ``g``) and ``mask = tokens != <pad>``:
``qs = tanh(g_in Wq[h]) / sqrt(K)``, ``s[l] = sum_k qs[k] tanh(h2[l] . Wk[h][:, k])`` and ``attention[n, i, h, :]``
the softmax of ``s`` over the positions with ``mask``: exactly 0.0 at ``<pad>``, all zeros for a sequence of
``<pad>`` only, and ``<sos>`` / ``<eos>`` are positions the model attends to (not masked).  These are the
operands the encoder's own attention used.  ``attention_top`` gives the ``k = attention_top_k`` largest weights of
every (block, head) row, descending, equal weights by ascending position (a stable sort); where a row has fewer
than ``k`` live positions the remaining entries are what that order gives for its zeros: value 0.0, the masked
positions in ascending order.  ``attention_top_k > L`` raises.  Both share the batch's single encoder pass with
every other output (the per-block states come from the encoder's taps); with neither requested no tap is
installed and none of this runs.  On the HIP backend they are ``pbx_attn_map_scores`` +
``pbx_attn_map_normalize`` (:func:`.ops.attention_maps.attention_maps`; ``key_dim = 64``, ``local_dim = 128``, at
most 8 heads, 8 blocks per launch pair) and ``pbx_row_topk``; elsewhere
:func:`.ops.attention_maps.attention_maps_torch`.  A **reference-semantics** model raises ``ValueError``: its
softmax runs over K identical query rows, so every weight is ``1/K`` by construction, ``Wq`` / ``Wk`` never
influence the model (they are non-persistent random buffers and the model computes the closed form), and a
constant would be returned as if it were a finding.  :meth:`Predictor.attention_map` is built on ``attention``.
"""
from __future__ import annotations

import os
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from .data.transforms import SimpleCharacterTokenizer, pad_to
from .data.vocab import ALL_AMINO_ACIDS, PAD_ID, SPECIAL_TOKENS, create_amino_acid_vocab
from .models.finetune import (ProteinBERTForSequenceClassification, ProteinBERTForTokenClassification,
                              load_finetuned_head)

OUTPUTS = ("global", "pooled", "residue", "go_probs", "go_topk", "residue_probs", "residue_tokens", "hidden_states",
           "residue_llr", "residue_logp", "residue_entropy", "pll", "attention", "attention_top")
SCORE_OUTPUTS = ("residue_llr", "residue_logp", "residue_entropy", "pll")
ATTENTION_OUTPUTS = ("attention", "attention_top")
SCORE_STRATEGIES = ("wt_marginal", "pll_ratio")
DEFAULT_OUTPUTS = ("global", "pooled", "go_topk")


TASK_PREFIXES = ("task:", "task_probs:")
_HEAD_NAME = re.compile(r"[A-Za-z][A-Za-z0-9_]*\Z")


def _task_request(o) -> Optional[Tuple[str, str]]:
    """``("task" | "task_probs", NAME)`` of a task output name, else None."""
    if isinstance(o, str):
        for p in TASK_PREFIXES:
            if o.startswith(p) and _HEAD_NAME.match(o[len(p):]):
                return p[:-1], o[len(p):]
    return None


def _check_outputs(outputs: Iterable[str], heads: Optional[dict] = None, semantics: Optional[str] = None) -> tuple:
    """The requested names as a tuple: the built-in ``OUTPUTS`` and ``task:NAME`` / ``task_probs:NAME`` of the
    registered ``heads``; anything else is ``unknown outputs``.  ``semantics``: the model's; the attention outputs
    of a reference-semantics model raise (there is no attention map to show)."""
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs)
    heads = heads or {}
    reqs = [_task_request(o) for o in outputs]
    bad = [o for o, r in zip(outputs, reqs) if o not in OUTPUTS and (r is None or r[1] not in heads)]
    if bad:
        tasks = tuple(p + n for n in heads for p in TASK_PREFIXES)
        raise ValueError(f"unknown outputs {bad}: expected a subset of {OUTPUTS + tasks}")
    for o, r in zip(outputs, reqs):
        if o not in OUTPUTS and r[0] == "task_probs" and _is_regression(heads[r[1]]):
            raise ValueError(f"{o}: {r[1]!r} is a regression head (n_classes == 1), it has values, not "
                             f"probabilities: request task:{r[1]}")
    asked = [o for o in outputs if o in ATTENTION_OUTPUTS]
    if asked and semantics is not None and semantics != "paper":
        raise ValueError(f"{asked}: a semantics={semantics!r} model has no attention map: its attention softmax "
                         f"runs over K identical query rows, so every weight is 1/K by construction and Wq / Wk "
                         f"never influence the model (it computes the closed form); attention maps exist for "
                         f"semantics='paper' models only")
    return outputs


def _is_regression(head) -> bool:
    return isinstance(head, ProteinBERTForSequenceClassification) and head.n_classes == 1


_SUBSTITUTION = re.compile(r"([A-Za-z])([0-9]+)([A-Za-z])\Z")
_AA_IDS = {c: len(SPECIAL_TOKENS) + i for i, c in enumerate(ALL_AMINO_ACIDS)}


def parse_variant(variant: str, sequence: str) -> List[Tuple[int, int]]:
    """``[(token position, new token id), ...]`` of a variant of ``sequence`` (the residues the model sees, so
    at most ``L - 2`` of them): one or more substitutions joined by ``:``, each ``<wild-type letter><1-based
    position><new letter>``, e.g. ``"A123G"`` or ``"A123G:L45P"``.  Residue ``i`` sits at token position ``i``
    (``<sos>`` is position 0).  ``ValueError`` naming the variant for bad syntax, a letter outside the
    vocabulary, a position outside the sequence, a wild-type letter that is not the sequence's, or a position
    given twice."""
    if not isinstance(variant, str) or not variant:
        raise ValueError(f"variant {variant!r}: expected substitutions such as 'A123G' joined by ':'")
    subs: List[Tuple[int, int]] = []
    for part in variant.split(":"):
        m = _SUBSTITUTION.match(part)
        if m is None:
            raise ValueError(f"variant {variant!r}: {part!r} is not <letter><position><letter>, e.g. 'A123G'")
        wt, pos, new = m.group(1), int(m.group(2)), m.group(3)
        for c in (wt, new):
            if c not in _AA_IDS:
                raise ValueError(f"variant {variant!r}: letter {c!r} is outside the vocabulary {ALL_AMINO_ACIDS}")
        if not 1 <= pos <= len(sequence):
            raise ValueError(f"variant {variant!r}: position {pos} is outside the sequence's {len(sequence)} "
                             f"scored residues")
        if sequence[pos - 1] != wt:
            raise ValueError(f"variant {variant!r}: the sequence has {sequence[pos - 1]!r} at position {pos}, "
                             f"not {wt!r}")
        if any(p == pos for p, _ in subs):
            raise ValueError(f"variant {variant!r}: position {pos} is given twice")
        subs.append((pos, _AA_IDS[new]))
    return subs


def _calls_torch(p: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(labels int32, their probabilities)`` over the last axis of ``p``: the first maximal index."""
    i = p.argmax(dim=-1)
    return i.to(torch.int32), p.gather(-1, i.unsqueeze(-1)).squeeze(-1)


def masked_mean_torch(h: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """fp32 mean of ``h [B, L, C]`` over the positions with ``tokens != <pad>``; zeros where there is none."""
    m = (tokens != PAD_ID).unsqueeze(-1)
    s = (h.float() * m).sum(dim=1)
    n = m.sum(dim=1)
    return torch.where(n > 0, s / n.clamp(min=1), torch.zeros_like(s))


def stable_topk_torch(p: torch.Tensor, k: int):
    """``(values [B, k], indices [B, k] int32)``: descending, equal values by ascending index."""
    v, i = torch.sort(p, dim=-1, descending=True, stable=True)
    return v[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()


class Predictor:
    """Inference on ``model`` (see the module docstring for the outputs and for how reference-semantics local
    predictions depend on the batch).  ``batch_size``: sequences per encoder pass of :meth:`predict`;
    ``device``: where the model runs (default: where its parameters are).  ``heads``: fine-tuned task heads by
    name (``[A-Za-z][A-Za-z0-9_]*``), each a :class:`~.models.ProteinBERTForTokenClassification` or
    :class:`~.models.ProteinBERTForSequenceClassification` whose ``.encoder`` is ``model``, or the path of a
    head file of ``cli finetune``, which is loaded around ``model`` (``head_meta[name]`` then holds the file's
    meta).  The head of an unfrozen fine-tune goes with its own encoder: ``Predictor(ft.encoder, heads={"ss":
    ft})``."""

    def __init__(self, model, batch_size: int = 256, device=None, heads: Optional[dict] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.model = model
        self.batch_size = int(batch_size)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.tokenizer = SimpleCharacterTokenizer(create_amino_acid_vocab(), add_sos_eos=True)
        self.heads: Dict[str, torch.nn.Module] = {}
        self.head_meta: Dict[str, Optional[dict]] = {}
        for name, head in (heads or {}).items():
            if not isinstance(name, str) or not _HEAD_NAME.match(name):
                raise ValueError(f"head name {name!r}: expected [A-Za-z][A-Za-z0-9_]*")
            meta = None
            if isinstance(head, (str, os.PathLike)):
                # freeze_encoder=False: building the head must not touch the model's requires_grad flags
                head, meta = load_finetuned_head(os.fspath(head), model, freeze_encoder=False)
            if not isinstance(head, (ProteinBERTForTokenClassification, ProteinBERTForSequenceClassification)):
                raise TypeError(f"head {name!r}: expected a fine-tuning model or the path of a head file, got "
                                f"{type(head).__name__}")
            if head.encoder is not model:
                raise ValueError(f"head {name!r} was built around another encoder: predict with "
                                 f"Predictor(head.encoder, heads={{{name!r}: head}})")
            self.heads[name] = head
            self.head_meta[name] = meta

    # ------------------------------------------------------------------------
    def tokenize(self, sequences: Sequence[str], truncate: bool = False) -> torch.Tensor:
        """``<sos>`` residues ``<eos>``, padded to ``model.sequences_length``: int64 ``[N, L]`` on the CPU.  A
        sequence of more than ``L - 2`` residues raises ``ValueError`` unless ``truncate`` keeps its first
        ``L - 2``."""
        L = self.model.sequences_length
        rows = []
        for n, s in enumerate(sequences):
            if not isinstance(s, str):
                raise TypeError(f"sequence {n}: expected a string, got {type(s).__name__}")
            if len(s) > L - 2:
                if not truncate:
                    raise ValueError(f"sequence {n} has {len(s)} residues, the model takes at most {L - 2} "
                                     f"(pass truncate=True to keep the first {L - 2})")
                s = s[:L - 2]
            rows.append(pad_to(self.tokenizer.encode_np(s), L))
        return torch.stack(rows) if rows else torch.zeros((0, L), dtype=torch.long)

    def _annotations(self, annotations, n: int, device) -> torch.Tensor:
        A = self.model.config["num_annotations"]
        if annotations is None:                     # "no GO prior", as models/finetune._split_inputs
            return torch.zeros((n, A), dtype=torch.float32, device=device)
        return annotations.to(device, non_blocking=True).float()

    # ------------------------------------------------------------------------
    def predict_batch(self, tokens: torch.Tensor, annotations: Optional[torch.Tensor] = None,
                      outputs: Iterable[str] = DEFAULT_OUTPUTS, go_top_k: int = 10,
                      attention_top_k: int = 10) -> Dict[str, torch.Tensor]:
        """One encoder pass over ``tokens [B, L]`` int64 (and ``annotations [B, A]``, zeros when None):
        the requested outputs as tensors on the model's device, without any host synchronisation."""
        outputs = _check_outputs(outputs, self.heads, self.model.semantics)
        model = self.model
        A = model.config["num_annotations"]
        if ("go_topk" in outputs) and not 1 <= go_top_k <= A:
            raise ValueError(f"go_top_k={go_top_k}: expected 1 .. {A}")
        if ("attention_top" in outputs) and not 1 <= attention_top_k <= tokens.shape[1]:
            raise ValueError(f"attention_top_k={attention_top_k}: expected 1 .. {tokens.shape[1]} (the sequence "
                             f"length)")
        tokens = tokens.to(self.device, non_blocking=True)
        ann = self._annotations(annotations, tokens.shape[0], self.device)
        # eval() for the model and the heads; every module's own flag is put back (a head holds the model as
        # its .encoder, so head.train(mode) alone would overwrite the model's)
        modes = [(m, m.training) for root in (model, *self.heads.values()) for m in root.modules()]
        model.eval()
        for head in self.heads.values():
            head.eval()
        try:
            with torch.no_grad():
                if model.resolved_backend(self.device) == "hip":
                    return self._predict_hip(tokens, ann, outputs, go_top_k, attention_top_k)
                return self._predict_torch(tokens, ann, outputs, go_top_k, attention_top_k)
        finally:
            for m, mode in modes:
                m.training = mode

    # ------------------------------------------------------------------------
    def _task_requests(self, outputs) -> Dict[str, set]:
        """Registered head name -> the kinds (``"task"``, ``"task_probs"``) requested of it."""
        req: Dict[str, set] = {}
        for o in outputs:
            r = None if o in OUTPUTS else _task_request(o)
            if r is not None:
                req.setdefault(r[1], set()).add(r[0])
        return req

    def _needs_all(self, req) -> bool:
        return any(self.heads[n].hidden == "all" for n in req)

    def _task_outputs(self, out, req, tokens, h, g, hs_all, gs_all, hip: bool) -> None:
        """The outputs of the requested task heads from this batch's encoder pass: ``h`` / ``g`` the final
        states, ``hs_all`` / ``gs_all`` every block's (filled only when a ``hidden="all"`` head asked)."""
        from .ops import finetune_head
        from .ops import infer_heads as ih
        for name, kinds in req.items():
            head = self.heads[name]
            every = head.hidden == "all"
            gfeat = torch.cat([x.float() for x in gs_all], dim=-1) if every else g.float()
            if isinstance(head, ProteinBERTForTokenClassification):
                hs = list(hs_all) if every else [h]
                gterm = head.global_head(gfeat) if head.global_head is not None else None       # [B, K]
                fn = (ih.token_head_calls if hip and finetune_head.supported_multi(hs, head.n_classes)
                      else ih.token_head_calls_torch)      # outside the kernel's range (K > 16, C != 128): torch
                P, lab, pmax = fn(hs, head.head.weight, head.head.bias, gterm, tokens,
                                  store_probs="task_probs" in kinds)
                if "task" in kinds:
                    out[f"task_{name}_labels"], out[f"task_{name}_label_probs"] = lab, pmax
                if "task_probs" in kinds:
                    out[f"task_{name}_probs"] = P
                continue
            z = head.head(gfeat).float()                                                        # [B, n]
            if head.n_classes == 1:
                out[f"task_{name}_values"] = z[:, 0]
                continue
            p = torch.softmax(z, dim=-1)
            if "task" in kinds:
                out[f"task_{name}_labels"], out[f"task_{name}_label_probs"] = _calls_torch(p)
            if "task_probs" in kinds:
                out[f"task_{name}_probs"] = p

    def _score_outputs(self, out, outputs, fn, h, tokens) -> None:
        """The requested ``SCORE_OUTPUTS`` of this batch's encoder pass through ``fn``
        (:func:`.ops.infer_heads.local_scores` or its torch definition); ``llr`` is stored only when
        ``residue_llr`` is requested."""
        if not any(o in outputs for o in SCORE_OUTPUTS):
            return
        lo = self.model.pretraining_local_output[0]
        llr, logp, ent, pll, n_live = fn(h, lo.weight, lo.bias, tokens, store_llr="residue_llr" in outputs)
        if "residue_llr" in outputs:
            out["residue_llr"] = llr
        if "residue_logp" in outputs:
            out["residue_logp"] = logp
        if "residue_entropy" in outputs:
            out["residue_entropy"] = ent
        if "pll" in outputs:
            out["pll"], out["n_residues"] = pll, n_live

    def _attention_outputs(self, out, outputs, hs, gs, g0, tokens, k, hip: bool) -> None:
        """``attention`` / ``attention_top_*`` from this batch's tapped states: ``hs[i]`` / ``gs[i]`` the outputs
        of block ``i``, ``g0`` the input layer's global output, so block ``i``'s query input is ``g0`` for
        ``i = 0`` and ``gs[i - 1]`` otherwise."""
        from .ops import attention_maps as am
        from .ops import infer_heads as ih
        atts = [blk.global_attention_layer for blk in self.model.proteinBERT_blocks]
        Wqs, Wks = [a.Wq for a in atts], [a.Wk for a in atts]
        if hip:
            hs = [h.contiguous() for h in hs]
        fn = am.attention_maps if hip and am.attention_supported(hs, Wks) else am.attention_maps_torch
        att = fn(hs, [g0] + list(gs[:-1]), Wqs, Wks, tokens)                      # [B, blocks, H, L]
        if "attention" in outputs:
            out["attention"] = att
        if "attention_top" in outputs:
            B, nb, H, L = att.shape
            rows = att.view(B * nb * H, L)
            v, i = (ih.row_topk(rows, k) if hip and att.is_cuda and ih.topk_supported(L, k)
                    else stable_topk_torch(rows, k))
            out["attention_top_values"], out["attention_top_indices"] = v.view(B, nb, H, k), i.view(B, nb, H, k)

    def _predict_hip(self, tokens, ann, outputs, k, att_k=10) -> Dict[str, torch.Tensor]:
        from .ops import infer_heads as ih
        from .ops.fused_model import fused_encode
        model = self.model
        tokens = tokens.contiguous()
        hidden_g: List[torch.Tensor] = []
        hidden_p: List[torch.Tensor] = []

        hs_all: List[torch.Tensor] = []       # references to every block's states, as _FinetuneBase._encode_all
        gs_all: List[torch.Tensor] = []
        want_hidden = "hidden_states" in outputs
        req = self._task_requests(outputs)
        want_att = any(o in outputs for o in ATTENTION_OUTPUTS)
        want_all = self._needs_all(req) or want_att
        g_first: List[torch.Tensor] = []

        def tap(i, h_i, g_i):
            if want_all:
                hs_all.append(h_i)
                gs_all.append(g_i)
            if want_hidden:
                hidden_g.append(g_i)
                hidden_p.append(ih.masked_mean_pool(h_i.contiguous(), tokens))  # one pool launch per block

        h, g, g_bf = fused_encode(model, tokens, ann, return_bf16=True,
                                  tap=tap if (want_hidden or want_all) else None,
                                  tap_input=g_first.append if want_att else None)
        h = h.contiguous()
        out: Dict[str, torch.Tensor] = {}
        if "global" in outputs:
            out["global"] = g
        if "pooled" in outputs:
            out["pooled"] = hidden_p[-1] if want_hidden else ih.masked_mean_pool(h, tokens)
        if "residue" in outputs:
            out["residue"] = h
        if "go_probs" in outputs or "go_topk" in outputs:
            go = model.pretraining_global_output[0]
            p = ih.go_probs(g_bf, go.weight, go.bias)
            if "go_probs" in outputs:
                out["go_probs"] = p
            if "go_topk" in outputs:
                v, i = ih.row_topk(p, k) if ih.topk_supported(p.shape[1], k) else stable_topk_torch(p, k)
                out["go_topk_values"], out["go_topk_indices"] = v, i
        if "residue_probs" in outputs or "residue_tokens" in outputs:
            P, tok, pmax = ih.local_probs(model, h, store_probs="residue_probs" in outputs)
            if "residue_probs" in outputs:
                out["residue_probs"] = P
            if "residue_tokens" in outputs:
                out["residue_tokens"], out["residue_token_probs"] = tok, pmax
        if want_hidden:
            out["hidden_global"] = torch.stack(hidden_g, dim=1)
            out["hidden_pooled"] = torch.stack(hidden_p, dim=1)
        self._score_outputs(out, outputs, ih.local_scores, h, tokens)
        self._task_outputs(out, req, tokens, h, g, hs_all, gs_all, hip=True)
        if want_att:
            self._attention_outputs(out, outputs, hs_all, gs_all, g_first[0], tokens, att_k, hip=True)
        return out

    def _predict_torch(self, tokens, ann, outputs, k, att_k=10) -> Dict[str, torch.Tensor]:
        model = self.model
        hidden_g: List[torch.Tensor] = []
        hidden_p: List[torch.Tensor] = []

        hs_all: List[torch.Tensor] = []
        gs_all: List[torch.Tensor] = []
        want_hidden = "hidden_states" in outputs
        req = self._task_requests(outputs)
        want_att = any(o in outputs for o in ATTENTION_OUTPUTS)
        want_all = self._needs_all(req) or want_att
        g_first: List[torch.Tensor] = []

        def tap(i, h_i, g_i):
            if want_all:
                hs_all.append(h_i)
                gs_all.append(g_i)
            if want_hidden:
                hidden_g.append(g_i.float())
                hidden_p.append(masked_mean_torch(h_i, tokens))

        h, g = model.encode_torch(tokens, ann, tap=tap if (want_hidden or want_all) else None,
                                  tap_input=g_first.append if want_att else None)
        out: Dict[str, torch.Tensor] = {}
        if "global" in outputs:
            out["global"] = g.float()
        if "pooled" in outputs:
            out["pooled"] = masked_mean_torch(h, tokens)
        if "residue" in outputs:
            out["residue"] = h
        heads = {"go_probs", "go_topk", "residue_probs", "residue_tokens"} & set(outputs)
        if heads:
            pl, pg = model.heads_torch(h, g)
            if "go_probs" in outputs:
                out["go_probs"] = pg
            if "go_topk" in outputs:
                out["go_topk_values"], out["go_topk_indices"] = stable_topk_torch(pg, k)
            if "residue_probs" in outputs:
                out["residue_probs"] = pl
            if "residue_tokens" in outputs:
                tok = pl.argmax(dim=-1)                                 # the first maximal index on ties
                out["residue_tokens"] = tok.to(torch.int32)
                out["residue_token_probs"] = pl.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
        if want_hidden:
            out["hidden_global"] = torch.stack(hidden_g, dim=1)
            out["hidden_pooled"] = torch.stack(hidden_p, dim=1)
        from .ops.infer_heads import local_scores_torch
        self._score_outputs(out, outputs, local_scores_torch, h, tokens)
        self._task_outputs(out, req, tokens, h, g, hs_all, gs_all, hip=False)
        if want_att:
            self._attention_outputs(out, outputs, hs_all, gs_all, g_first[0], tokens, att_k, hip=False)
        return out

    # ------------------------------------------------------------------------
    def predict(self, sequences: Union[Sequence[str], torch.Tensor], annotations: Optional[torch.Tensor] = None,
                outputs: Iterable[str] = DEFAULT_OUTPUTS, go_top_k: int = 10,
                truncate: bool = False, attention_top_k: int = 10) -> Dict[str, torch.Tensor]:
        """Predictions for ``sequences`` (a list of strings, tokenised by :meth:`tokenize`; or an int64 token
        tensor ``[N, L]``, taken as it is) in batches of ``batch_size``: CPU tensors in input order.  No host
        synchronisation per batch: every batch's outputs are copied, without blocking, into host tensors
        allocated once (pinned when the model is on a GPU), and the device is synchronised once at the end.
        ``go_top_k`` / ``attention_top_k``: the ``k`` of the ``go_topk`` / ``attention_top`` outputs."""
        outputs = _check_outputs(outputs, self.heads, self.model.semantics)
        tokens = sequences if isinstance(sequences, torch.Tensor) else self.tokenize(list(sequences), truncate)
        if tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise ValueError("token input must be an int64 [N, L] tensor")
        N = tokens.shape[0]
        if annotations is not None and annotations.shape[0] != N:
            raise ValueError(f"{annotations.shape[0]} annotation rows for {N} sequences")
        cuda = self.device.type == "cuda"
        host: Dict[str, torch.Tensor] = {}
        for s in range(0, N, self.batch_size):
            e = min(N, s + self.batch_size)
            out = self.predict_batch(tokens[s:e], None if annotations is None else annotations[s:e], outputs,
                                     go_top_k, attention_top_k)
            for name, t in out.items():
                if name not in host:
                    host[name] = torch.empty((N,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=cuda)
                host[name][s:e].copy_(t, non_blocking=True)
        if cuda:
            torch.cuda.synchronize(self.device)
        return host

    # ------------------------------------------------------------------------
    def _wild_type(self, wild_type: str, truncate: bool) -> Tuple[torch.Tensor, str]:
        """``(tokens [1, L], the residues that are scored)`` of one sequence."""
        if not isinstance(wild_type, str):
            raise TypeError(f"expected a sequence string, got {type(wild_type).__name__}")
        tokens = self.tokenize([wild_type], truncate)
        return tokens, wild_type[:self.model.sequences_length - 2]

    def score_variants(self, wild_type: str, variants: Sequence[str], strategy: str = "wt_marginal",
                       truncate: bool = False) -> dict:
        """Scores of substitution variants of ``wild_type`` (``"A123G"``, ``"A123G:L45P"``: see
        :func:`parse_variant`; any malformed one raises ``ValueError`` naming it, before the encoder runs).

        ``strategy="wt_marginal"``: one encoder pass over the wild type; a variant's score is the sum of
        ``residue_llr[pos, new]`` over its substitutions, gathered on the device and read once.
        ``strategy="pll_ratio"``: every variant goes through the encoder (batches of ``batch_size``, only the
        ``pll`` output, so no ``llr`` is stored) and its score is ``pll(variant) - pll(wild type)``.

        Returns ``{"scores": fp32 [n], "variants": list, "strategy": str, "wild_type_pll": float}``."""
        if strategy not in SCORE_STRATEGIES:
            raise ValueError(f"strategy {strategy!r}: expected one of {SCORE_STRATEGIES}")
        variants = list(variants)
        tokens, seq = self._wild_type(wild_type, truncate)
        subs = [parse_variant(v, seq) for v in variants]
        n = len(variants)
        width = max([len(s) for s in subs], default=1)
        # [n, width] index matrices, short variants padded with (position 0, token 0) under a zero mask
        pos = torch.zeros((n, width), dtype=torch.long)
        new = torch.zeros((n, width), dtype=torch.long)
        mask = torch.zeros((n, width), dtype=torch.float32)
        for i, s in enumerate(subs):
            for j, (p, a) in enumerate(s):
                pos[i, j], new[i, j], mask[i, j] = p, a, 1.0
        if strategy == "wt_marginal":
            out = self.predict_batch(tokens, outputs=("residue_llr", "pll"))
            dev = out["residue_llr"].device
            picked = out["residue_llr"][0][pos.to(dev), new.to(dev)] * mask.to(dev)        # [n, width]
            both = torch.cat([picked.sum(dim=1), out["pll"]]).cpu()                        # the one host read
            scores, wt_pll = both[:n].clone(), float(both[n])
        else:
            rows = tokens.repeat(n + 1, 1)                       # row 0 stays the wild type
            live = mask.bool()
            rows[1:][torch.arange(n).unsqueeze(1).expand(n, width)[live], pos[live]] = new[live]
            pll = self.predict(rows, outputs=("pll",))["pll"]
            scores, wt_pll = pll[1:] - pll[0], float(pll[0])
        return {"scores": scores, "variants": variants, "strategy": strategy, "wild_type_pll": wt_pll}

    def mutation_scan(self, sequence: str, truncate: bool = False) -> dict:
        """The deep mutational scan of one sequence from a single encoder pass: ``llr [n_res, 22]`` (the
        log-odds of every substitution at every residue position, without ``<sos>`` / ``<eos>``; columns in
        the order of ``letters`` = ``data.vocab.ALL_AMINO_ACIDS``), ``logp [n_res]``, ``entropy [n_res]``,
        ``pll`` (float) and ``letters``, as CPU tensors."""
        tokens, seq = self._wild_type(sequence, truncate)
        out = self.predict_batch(tokens, outputs=("residue_llr", "residue_logp", "residue_entropy", "pll"))
        n_res = len(seq)
        cols = torch.tensor(self.tokenizer.vocab.lookup_indices(ALL_AMINO_ACIDS), device=out["pll"].device)
        rows = slice(1, 1 + n_res)                               # position 0 is <sos>
        return {"llr": out["residue_llr"][0, rows].index_select(-1, cols).cpu(),
                "logp": out["residue_logp"][0, rows].cpu(), "entropy": out["residue_entropy"][0, rows].cpu(),
                "pll": float(out["pll"][0]), "letters": ALL_AMINO_ACIDS}

    def attention_map(self, sequence: str, truncate: bool = False) -> dict:
        """Where the model looks on one sequence, from a single encoder pass (paper semantics only; a
        reference-semantics model raises ``ValueError``, see the module docstring): ``attention [blocks, H,
        n + 2]`` (the weights of every block and head over the ``<sos>``, residue and ``<eos>`` columns, the
        ``<pad>`` columns trimmed: every row sums to 1), ``per_block [blocks, n + 2]`` (the sum over the heads)
        and ``letters`` (the ``n + 2`` column labels: ``"<sos>"``, the residues, ``"<eos>"``), as CPU tensors."""
        _check_outputs(("attention",), self.heads, self.model.semantics)        # before the sequence is touched
        tokens, seq = self._wild_type(sequence, truncate)
        att = self.predict_batch(tokens, outputs=("attention",))["attention"][0, :, :, :len(seq) + 2].cpu()
        return {"attention": att, "per_block": att.sum(dim=1), "letters": ["<sos>"] + list(seq) + ["<eos>"]}
