"""vibrato_amd: MI355X (gfx950) native batched Viterbi tokenizer, a drop-in for the
tokenize() path of daac-tools/vibrato.  The compute lives in csrc/ (HIP kernels + C ABI,
built into lib/libvibrato_hip.so); this package is the thin host mirror of vibrato's
Dictionary / Tokenizer / Worker / Token API."""
from .api import (Batch, Dictionary, Format, Marginal, NBest, Samples, SystemDictionaryBuilder, Token, Tokenizer, VibratoError, Worker,  # noqa: F401
                  Workspace, MARGINAL_NODE_DTYPE, TOKEN_DTYPE, LEX_NAMES, compute_connid_probs)
from ._native import DETAIL_ROUND, FORMAT_ROUND, MECAB_ROUND, SPLIT_TILE, WAKATI_ROUND  # noqa: F401

__all__ = ["DETAIL_ROUND", "FORMAT_ROUND", "Format", "MECAB_ROUND", "SPLIT_TILE", "WAKATI_ROUND", "Batch", "Dictionary", "Marginal", "NBest", "Samples", "SystemDictionaryBuilder", "Token", "Tokenizer", "VibratoError", "Worker",
           "Workspace", "MARGINAL_NODE_DTYPE", "TOKEN_DTYPE", "LEX_NAMES", "compute_connid_probs"]
