"""Model families: ProteinBERT pretraining model and fine-tuning heads."""
from .proteinbert import ProteinBERT, ProteinBERTBlock, GlobalAttention, GlobalAttentionHead, build_model
from .finetune import (ProteinBERTForTokenClassification, ProteinBERTForSequenceClassification, build_finetune_model,
                       load_finetuned_head)

__all__ = ["ProteinBERT", "ProteinBERTBlock", "GlobalAttention", "GlobalAttentionHead", "build_model",
           "ProteinBERTForTokenClassification", "ProteinBERTForSequenceClassification", "build_finetune_model",
           "load_finetuned_head"]
