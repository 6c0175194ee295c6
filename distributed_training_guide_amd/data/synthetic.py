"""Synthetic causal-LM dataset: deterministic random token rows of the same
shape the reference's pipeline produces ({input_ids, attention_mask, labels},
labels = input_ids — /root/reference/01-single-gpu/train_llm.py:221-235).

BASELINE.json mandates synthetic data / random-init weights (no network for
datasets or checkpoints); rows are reproducible per (seed, index) so resume
and determinism tests behave like a real on-disk dataset.
"""
import torch
from torch.utils.data import Dataset

from ..ops.doc_mask import doc_start_from_ids


class SyntheticTextDataset(Dataset):
    """doc_len > 0 turns each row into packed documents: an EOS id
    (vocab_size - 1) is written at pseudo-random gaps of that mean,
    deterministically per (seed, index).  doc_mask adds the row's
    "doc_start" int32 [S] (ops/doc_mask.py).  doc_len = 0 leaves the rows
    bit-identical to the plain random ones."""

    def __init__(self, vocab_size: int, seq_length: int,
                 num_samples: int = 4096, seed: int = 0, doc_len: int = 0,
                 doc_mask: bool = False):
        if doc_len < 0:
            raise ValueError("doc_len must be >= 0")
        self.vocab_size = vocab_size
        self.seq_length = seq_length
        self.num_samples = num_samples
        self.seed = seed
        self.doc_len = doc_len
        self.doc_mask = doc_mask
        self.eos_id = vocab_size - 1

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + idx)
        ids = torch.randint(0, self.vocab_size, (self.seq_length,),
                            generator=g, dtype=torch.long)
        if self.doc_len > 0:
            # document lengths uniform in [1, 2*doc_len - 1] (mean doc_len),
            # drawn after the tokens so those match the doc_len=0 row; the
            # EOS id may also occur among the random tokens, which only
            # makes a few documents shorter
            n = self.seq_length
            lens = torch.randint(1, 2 * self.doc_len, (n,), generator=g)
            eos_pos = torch.cumsum(lens, 0) - 1
            ids[eos_pos[eos_pos < n]] = self.eos_id
        row = {
            "input_ids": ids,
            "attention_mask": torch.ones(self.seq_length, dtype=torch.long),
            "labels": ids.clone(),
        }
        if self.doc_mask:
            row["doc_start"] = doc_start_from_ids(ids[None], self.eos_id)[0]
        return row


def default_collate(batch):
    """Stack dict rows — the reference uses transformers'
    default_data_collator (01:69); same behavior for our fixed-length rows."""
    out = {}
    for k in batch[0]:
        out[k] = torch.stack([row[k] for row in batch])
    return out
