"""TEST INFRASTRUCTURE: restatements of the skip-connection arithmetic of SerializedUnpooling (ptv3.py:42-100, :607-626) that
tests/test_cpu_skip.py and tests/test_gpu_skip.py compare against.  Plain torch on the CPU, never imported by the product.

  fft_filter(x, s, dtype)    the reference's Fourier_filter for x (N, C) with threshold 1, written from its description: 2-D FFT
                             over (C, N), fftshift, the two centre columns N // 2 - 1, N // 2 of the row-frequency axis times a
                             mask value held in float32, inverse, real part.  dtype float32 is the reference's own arithmetic.
  closed_filter(x, s, ...)   the closed form in fp64: y = x + k (S0 + A cos t + B sin t), k = (float32(s) - 1) / N.
  stats(x, ref, n_total)     [S0 A B] (3 C) fp64.
  merge(...)                 what cdseg_skip_merge computes, in fp64.
"""
import math

import numpy as np
import torch


def fft_filter(x, s, dtype=torch.float64, round_s=True):
    v = x.to(dtype).t().unsqueeze(0)  # (1, C, N)
    fr = torch.fft.fftshift(torch.fft.fftn(v, dim=(-2, -1)), dim=(-2, -1))
    n = v.shape[-1]
    mask = torch.ones(v.shape, dtype=torch.float32 if round_s else torch.float64)
    mask[..., n // 2 - 1:n // 2 + 1] = s
    fr = fr * mask
    out = torch.fft.ifftn(torch.fft.ifftshift(fr, dim=(-2, -1)), dim=(-2, -1)).real
    return out.squeeze(0).t()


def angles(n, ref=None, n_total=None):
    """(cos, sin) (n) fp64 of 2 pi m / N at m = ref[r] (None: r)."""
    n_total = n if n_total is None else n_total
    m = torch.arange(n, dtype=torch.float64) if ref is None else ref.double()
    t = 2.0 * math.pi * m / n_total
    return torch.cos(t), torch.sin(t)


def stats(x, ref=None, n_total=None):
    x = x.double()
    cs, sn = angles(x.shape[0], ref, n_total)
    return torch.cat([x.sum(0), (x * cs[:, None]).sum(0), (x * sn[:, None]).sum(0)])


def k_of(s, n_total, round_s=True):
    return ((float(np.float32(s)) if round_s else float(s)) - 1.0) / n_total


def wave(st, n, ref=None, n_total=None):
    """(n, C) fp64: S0 + A cos t_r + B sin t_r for st = [S0 A B]."""
    c = st.numel() // 3
    cs, sn = angles(n, ref, n_total)
    return st[:c][None] + cs[:, None] * st[c:2 * c][None] + sn[:, None] * st[2 * c:][None]


def closed_filter(x, s, ref=None, n_total=None, round_s=True):
    n = x.shape[0]
    n_total = n if n_total is None else n_total
    return x.double() + k_of(s, n_total, round_s) * wave(stats(x, ref, n_total), n, ref, n_total)


def merge(x, st=None, s=1.0, f=1.0, ref=None, n_total=None, child=None, cluster=None, folded=False):
    n = x.shape[0]
    n_total = n if n_total is None else n_total
    v = x.double()
    if st is not None:
        t = k_of(s, n_total) * wave(st.double(), n, ref, n_total)
        v = v + f * t if folded else f * (v + t)
    else:
        v = f * v
    if child is not None:
        v = v + child.double()[cluster.long()]
    return v
