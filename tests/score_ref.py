"""fp64 reference of the per-token negative log-likelihood: nll = logsumexp(logits) - logits[token]."""
import numpy as np
import torch


def nll_ref(logits, tokens) -> np.ndarray:
    """logits [..., V] (any float type), tokens [...] integer -> fp64 nll [...]."""
    lg = torch.as_tensor(np.asarray(logits)).to(torch.float64)
    tk = torch.as_tensor(np.asarray(tokens)).to(torch.int64)
    return (torch.logsumexp(lg, dim=-1) - lg.gather(-1, tk[..., None])[..., 0]).numpy()


def fused_bound(nll, V) -> np.ndarray:
    """|fused fp32 loss - fp64 loss of the same fp32 logits|, worst case over any summation order: V terms of at most 1 with a sum of at least 1
    (exp, add), and the final log / subtraction relative to the result."""
    return (V + 64) * 2.0 ** -24 + 2.0 ** -22 * np.abs(nll)
