"""ORACLE — test infrastructure only (never imported by the product path).

High-precision restatements of the two kernels every trained parameter passes through at the
end of a step (include/ttmi.h): the fused AdamW (``ttmi_adamw*``) and the generic split fold
(``ttmi_fold_desc``).  Plain numpy on the CPU:

  adamw_step64     torch.optim.AdamW (non-amsgrad, decoupled weight decay) in float64
  fold64           the fold's sum in float64 (int64 partials: the exact integer total)
  fold32_in_order  the same sum as sequential float32 adds in split order, bit for bit what the
                   kernel guarantees for S <= 16 and for int64 partials
  HYPERS           the hyper-parameter sets the optimizer tests use ({lr, beta1, beta2, eps, wd},
                   the layout of the device ``hyper`` array)
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

HYPERS = ((1e-3, 0.9, 0.999, 1e-8, 0.01),
          (1e-4, 0.9, 0.999, 1e-8, 0.0),
          (3e-2, 0.5, 0.9, 1e-3, 0.1))


def adamw_step64(p, g, m, v, hyper: Sequence[float], t: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One AdamW step at step count ``t`` (>= 1) with hyper = (lr, beta1, beta2, eps,
    weight_decay); returns the new (p, m, v) as float64 arrays (inputs untouched)."""
    lr, b1, b2, eps, wd = (float(x) for x in hyper)
    p = np.asarray(p, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def _slabs(parts, S: int, s_stride: int, M: int, N: int) -> np.ndarray:
    """[S, M, N] view of the partials read: part[s*s_stride + m*N + n]."""
    parts = np.asarray(parts).reshape(-1)
    if S <= 0 or s_stride < M * N or parts.size < (S - 1) * s_stride + M * N:
        raise ValueError("fold: partials too short for S, s_stride, M, N")
    return np.stack([parts[s * s_stride: s * s_stride + M * N].reshape(M, N) for s in range(S)])


def fold64(parts, S: int, s_stride: int, M: int, N: int, c: Optional[np.ndarray], accumulate: int,
           fx_shift: int) -> np.ndarray:
    """The ttmi_fold_desc contract in float64: Σ_s part[s*s_stride + m*N + n], plus ``c`` [M, N]
    when accumulate bit 0 is set.  fx_shift > 0: ``parts`` is int64 fixed point, summed exactly
    in int64 and scaled by 2^-fx_shift (exact in float64 below 2^53 units)."""
    sl = _slabs(parts, S, s_stride, M, N)
    if fx_shift > 0:
        if sl.dtype != np.int64:
            raise TypeError("fold64: fixed-point partials are int64")
        tot = np.ldexp(sl.sum(axis=0, dtype=np.int64).astype(np.float64), -fx_shift)
    else:
        tot = sl.astype(np.float64).sum(axis=0)
    if accumulate & 1:
        tot = np.asarray(c, dtype=np.float64).reshape(M, N) + tot
    return tot


def fold32_in_order(parts, S: int, s_stride: int, M: int, N: int, c: Optional[np.ndarray],
                    accumulate: int, fx_shift: int) -> np.ndarray:
    """The same sum as the kernel's narrow regime computes it, in float32: 0 + part[0] + part[1]
    + ... in split order, then c + sum when accumulate bit 0 is set.  fx_shift > 0: the sum is
    float32(float64(Σq)·2^-fx_shift), one rounding of the exact integer total."""
    sl = _slabs(parts, S, s_stride, M, N)
    if fx_shift > 0:
        if sl.dtype != np.int64:
            raise TypeError("fold32_in_order: fixed-point partials are int64")
        tot = np.ldexp(sl.sum(axis=0, dtype=np.int64).astype(np.float64), -fx_shift).astype(np.float32)
    else:
        tot = np.zeros((M, N), dtype=np.float32)
        for s in range(S):
            tot = tot + sl[s].astype(np.float32)
    if accumulate & 1:
        tot = np.asarray(c, dtype=np.float32).reshape(M, N) + tot
    return tot.astype(np.float32)
