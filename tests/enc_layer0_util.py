"""Shared by the encoder layer-0 tests (test_enc_layer0_scheme.py on the CPU,
test_gpu_enc_layer0.py on the GPU): the materialised reference of the layer
the engine runs in closed form (csrc/attention.hip enc_attention_rank2_kernel),
and the inputs that stress that closed form.

The layer, as the reference model computes it (encoder/transformer.py: the
Linear(1, d) embedding, the layer's LayerNorm, multi_headed_attn.py up to the
context before W_o):

    x = s w + b;  LN(x) (eps 1e-6);  q | k | v = LN(x) Wqkv^T + bqkv;
    8 heads of 32, q / sqrt(32);  key mask signal == 0 filled with -1e18;
    softmax;  context.

Keys at or past a chunk's span do not exist for it (each chunk is computed on
its own first span samples), rows at or past span are NaN here and are not
compared.
"""
import math

import numpy as np
import torch

D, H, DH = 256, 8, 32
LN_EPS = 1e-6
MASK_FILL = -1e18


def materialised(signal, span, w_in, b_in, wqkv, bqkv, ln_g, ln_b, dtype=torch.float64):
    """The layer materialised in `dtype` on the CPU: [B, T, 256], rows t >= span NaN.
    dtype float64 is the reference; float32 is the reference model's own
    arithmetic, whose error against float64 is the yardstick E32."""
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
    sig, w, b, W, bq, g, be = map(c, (signal, w_in, b_in, wqkv, bqkv, ln_g, ln_b))
    B, T = sig.shape
    out = torch.full((B, T, D), float("nan"), dtype=dtype)
    for i in range(B):
        L = min(int(span[i]), T)
        if L <= 0:
            continue
        s = sig[i, :L]
        x = s[:, None] * w + b
        xn = torch.nn.functional.layer_norm(x, (D,), g, be, LN_EPS)
        q, k, v = (xn @ W.T + bq).view(L, 3, H, DH).permute(1, 2, 0, 3)  # each [H, L, 32]
        sc = (q / math.sqrt(DH)) @ k.transpose(1, 2)
        sc = sc.masked_fill((s == 0)[None, None, :], MASK_FILL)
        out[i, :L] = (torch.softmax(sc, -1) @ v).permute(1, 0, 2).reshape(L, D)
    return out


def centred(v):
    return v - v.mean()


def collinear_bias(w, cos, rng):
    """A zero-mean b' [256] (double) of |w'|'s norm at the given cosine to w' = w - mean(w)."""
    wc = centred(np.asarray(w, np.float64).reshape(-1))
    u = centred(rng.standard_normal(wc.size))
    u -= wc * (u @ wc) / (wc @ wc)
    u *= np.linalg.norm(wc) / np.linalg.norm(u)
    return cos * wc + math.sqrt(max(0.0, 1.0 - cos * cos)) * u


def make_weights(cos, seed, qk_scale=1.0, w_mean=0.0, w_dev=0.5, b_zero=False, w_const=False):
    """fp32 numpy weights of the layer with a prescribed cosine between the
    centred embedding weight w' and bias b' (|b'| = |w'|, so the variance's
    minimum sits at s0 = -cos).  cos=None leaves b random (cos ~ 0)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(D) * w_dev
    wc = w - w.mean()
    bc = collinear_bias(wc, cos, rng) if cos is not None else centred(rng.standard_normal(D)) * w_dev
    b = bc + 0.1
    w = wc + w_mean
    if w_const:
        w = np.full(D, 10.0)
    if b_zero:
        b = np.zeros(D)
    wqkv = rng.standard_normal((3 * D, D)) / math.sqrt(D)
    wqkv[:2 * D] *= qk_scale
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(w_in=f(w), b_in=f(b), wqkv=f(wqkv), bqkv=f(rng.standard_normal(3 * D) * 0.1),
                ln_g=f(1.0 + 0.1 * rng.standard_normal(D)), ln_b=f(0.1 * rng.standard_normal(D)))


def measured_cos_s0(wts):
    """(cos(w', b'), s0 = -m_wb / m_ww) of the fp32 weights, in double."""
    w, b = wts["w_in"].astype(np.float64), wts["b_in"].astype(np.float64)
    wc, bc = w - w.mean(), b - b.mean()
    ww = wc @ wc
    if ww == 0.0:
        return 0.0, 0.0
    nb = np.linalg.norm(bc)
    return (float(wc @ bc / math.sqrt(ww) / nb) if nb else 0.0), float(-(wc @ bc) / ww)


def clustered_signal(B, T, s0, seed, scale=1.0):
    """[B, T] fp32: standard normal samples (times scale), every third one
    within +-0.05 of s0 instead (where the expanded variance cancels)."""
    rng = np.random.default_rng(seed)
    sig = rng.standard_normal((B, T)) * scale
    near = s0 + rng.uniform(-0.05, 0.05, (B, T))
    sig[:, ::3] = near[:, ::3]
    sig = sig.astype(np.float32)
    sig[sig == 0] = np.float32(1e-3)  # no accidental mask
    return sig
