"""Shared by the encoder-attention tests (test_enc_attn_scheme.py on the CPU,
test_gpu_enc_attention.py on the GPU): the plain reference of the attention
that encoder layers 1 and 2 run (csrc/attention.hip enc_attention_h3_kernel,
and enc_attention_kernel under exact_fp32), a numpy model of the split-fp16
kernel's arithmetic, the bar both test files hold results to, and the cases.

The operation, as the reference model computes it (multi_headed_attn.py:154-177
under the encoder's key mask, encoder/transformer.py:117-121), on rows
q | k | v of qkv [B * T, 768]:

    8 heads of 32;  scores = (q / sqrt(32)) k^T;  keys with signal == 0 filled
    with -1e18;  softmax;  context = weights v.

Keys and queries at t >= span do not exist for a chunk (each chunk is computed
on its own first span rows); rows at or past span are NaN here and are not
compared.  1 <= span throughout: span = 0 is outside the kernels' contract.

No GPU and nothing compiled is imported here.
"""
import functools
import math

import numpy as np
import torch

D, H, DH = 256, 8, 32
MASK_FILL = -1e18
ENC_THR = 8.0          # attention.hip: the lazy running maximum's threshold, log2 units
TILE = 32              # keys per tile
F16_LIMIT = 65504.0
Q_LIMIT = F16_LIMIT * math.sqrt(DH) / math.log2(math.e)   # a query element whose scaled value reaches the fp16 limit

# The bar (test_gpu_enc_attention.py's docstring derives it).  R_EMU is the
# bound test_enc_attn_scheme.py holds the emulation to, in units of
# max(E32, FLOOR max|V|); K follows from it (4, or 5 R_EMU beyond 0.8) and was
# fixed from the CPU emulation alone, before any kernel output was looked at.
R_EMU = 0.8
K_BAR = 4.0 if R_EMU <= 0.8 else 5.0 * R_EMU
FLOOR = 2.0 ** -21     # a value split as fp16 hi + lo keeps 22 bits; both P and V are split

DROPS = ("K_lo.Q_hi", "K_hi.Q_lo", "V_lo.P_hi", "V_hi.P_lo")


# ----------------------------------------------------------------- reference
def reference(qkv, sig, span, dtype=torch.float64):
    """The attention in `dtype` on the CPU: [B, T, 256], rows t >= span NaN.
    float64 is the reference; float32 is the reference model's own arithmetic,
    whose error against float64 is the yardstick E32."""
    sig = torch.as_tensor(sig).detach().cpu()
    B, T = sig.shape
    rows = torch.as_tensor(qkv).detach().cpu().to(dtype).view(B, T, 3, H, DH)
    out = torch.full((B, T, D), float("nan"), dtype=dtype)
    for b in range(B):
        L = min(int(span[b]), T)
        if L <= 0:
            continue
        q, k, v = rows[b, :L].permute(1, 2, 0, 3)          # each [H, L, 32]
        sc = (q / math.sqrt(DH)) @ k.transpose(1, 2)
        sc = sc.masked_fill((sig[b, :L] == 0)[None, None, :], MASK_FILL)
        out[b, :L] = (torch.softmax(sc, -1) @ v).permute(1, 0, 2).reshape(L, D)
    return out


# ----------------------------------------------------------------- the shipped scheme
def _split(x):
    """fp32 x -> (hi, lo) as float64 arrays holding fp16 values: hi = fp16(x), lo = fp16(x - hi)."""
    x = x.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _dropped(drop, term, step):
    return drop is not None and drop[0] == term and drop[1] in (None, step)


def emulate_h3(qkv, sig, span, drop=None):
    """A numpy model of enc_attention_h3_kernel's arithmetic, written from the
    kernel's comments: [B, T, 256] float32, rows t >= span NaN.

    Scores in log2 units: the fp32 product q * (log2(e) / sqrt(32)) is split
    into fp16 hi + lo, K and V are split the same way, and a product is
    hi*hi + hi*lo + lo*hi summed over a tile of 32 keys (two k-steps of 16:
    head dims for the scores, keys for P.V) and rounded to fp32 once per tile
    (the MFMA's own summation order is not modelled).  Masked keys score
    -1e18, keys past the span -inf.  The running maximum is lazy: a block of
    32 queries (a lane carries a query at or past the span as a copy of row
    span - 1) rescales O and l only when one of its tile maxima exceeds its m
    by more than ENC_THR.  p = 2^(s - m) in fp32, split into hi + lo for P.V;
    the row sum and O accumulate in fp32.

    drop = (term, step): term of DROPS is left out, on k-step `step` of every
    tile or, step None, on both.
    """
    sig = np.asarray(sig, np.float32)
    B, T = sig.shape
    rows = np.asarray(qkv, np.float32).reshape(B, T, 3, H, DH)
    qs = np.float32(np.float32(1.4426950408889634) / np.float32(math.sqrt(DH)))
    out = np.full((B, T, D), np.nan, np.float32)
    for b in range(B):
        L = min(int(span[b]), T)
        nkt = (L + TILE - 1) // TILE
        nq = nkt * TILE
        qi = np.minimum(np.arange(nq), L - 1)
        ki = np.minimum(np.arange(nq), L - 1)
        live = np.arange(nq) < L
        qh, ql = _split(rows[b, qi, 0].transpose(1, 0, 2) * qs)                  # [H, nq, 32]
        kh, kl = _split(np.where(live[:, None, None], rows[b, ki, 1], 0).transpose(1, 0, 2))
        vh, vl = _split(np.where(live[:, None, None], rows[b, ki, 2], 0).transpose(1, 0, 2))
        fill = np.where(live, np.where(sig[b, ki] == 0, MASK_FILL, 0.0), -np.inf)  # per key; 0: keep the score
        o = np.zeros((H, nq, DH), np.float32)
        m = np.full((H, nq), -np.inf, np.float32)
        l = np.zeros((H, nq), np.float32)
        for kt in range(nkt):
            ks = slice(kt * TILE, (kt + 1) * TILE)
            s = np.zeros((H, nq, TILE))
            for st in range(2):
                d = slice(16 * st, 16 * st + 16)
                kht, klt = kh[:, ks, d].transpose(0, 2, 1), kl[:, ks, d].transpose(0, 2, 1)
                s += qh[:, :, d] @ kht
                if not _dropped(drop, "K_hi.Q_lo", st):
                    s += ql[:, :, d] @ kht
                if not _dropped(drop, "K_lo.Q_hi", st):
                    s += qh[:, :, d] @ klt
            s = s.astype(np.float32)
            f = fill[ks]
            s = np.where(f == 0.0, s, f.astype(np.float32)[None, None, :])
            mx = s.max(-1)
            with np.errstate(invalid="ignore"):
                trig = (mx > m + np.float32(ENC_THR)).reshape(H, nkt, TILE).any(-1)   # per block of 32 queries
                trig = np.repeat(trig, TILE, axis=1)
                mn = np.where(trig, np.maximum(m, mx), m)
                alpha = np.where(trig, np.exp2(np.where(trig, m - mn, 0).astype(np.float32)), np.float32(1.0))
                m = mn
                l = (l * alpha).astype(np.float32)
                o = (o * alpha[:, :, None]).astype(np.float32)
                p = np.exp2((s - m[:, :, None]).astype(np.float32)).astype(np.float32)
            l = (l + p.sum(-1, dtype=np.float64)).astype(np.float32)
            ph, pl = _split(p)
            acc = np.zeros((H, nq, DH))
            for st in range(2):
                kk = slice(kt * TILE + 16 * st, kt * TILE + 16 * st + 16)
                pk = slice(16 * st, 16 * st + 16)
                acc += ph[:, :, pk] @ vh[:, kk]
                if not _dropped(drop, "V_hi.P_lo", st):
                    acc += pl[:, :, pk] @ vh[:, kk]
                if not _dropped(drop, "V_lo.P_hi", st):
                    acc += ph[:, :, pk] @ vl[:, kk]
            o = (o + acc).astype(np.float32)
        inv = (np.float32(1.0) / l).astype(np.float32)
        out[b, :L] = (o * inv[:, :, None]).astype(np.float32)[:, :L].transpose(1, 0, 2).reshape(L, D)
    return out


# ----------------------------------------------------------------- the bar
def yardsticks(case):
    """(ref fp64 [B, T, 256] numpy, live mask, E32, max|ref|, max|V| over live rows) of a case, computed once."""
    if "_ref" not in case:
        ref = reference(case["qkv"], case["sig"], case["span"]).numpy()
        f32 = reference(case["qkv"], case["sig"], case["span"], torch.float32).numpy().astype(np.float64)
        live = ~np.isnan(ref)
        B, T = case["sig"].shape
        v = np.abs(case["qkv"].reshape(B, T, 3, D)[:, :, 2].astype(np.float64))
        case["_ref"] = (ref, live, float(np.abs(f32 - ref)[live].max()), float(np.abs(ref[live]).max()),
                        float(v[live].max()))
    return case["_ref"]


def bars(case):
    """(K max(E32, 2^-21 max|V|), the old ceiling 1e-4 max(1, max|ref| / 4)) of a case."""
    _, _, e32, mx, vmax = yardsticks(case)
    return K_BAR * max(e32, FLOOR * vmax), 1e-4 * max(1.0, mx / 4.0)


def error(case, out):
    """max |out - fp64| over the live rows of out [B, T, 256]."""
    ref, live, *_ = yardsticks(case)
    return float(np.abs(np.asarray(out, np.float64).reshape(ref.shape) - ref)[live].max())


# ----------------------------------------------------------------- cases
def _case(name, qkv, sig, span):
    B, T = sig.shape
    assert qkv.shape == (B * T, 3 * D) and min(span) >= 1 and max(span) <= T, name
    return dict(name=name, qkv=np.ascontiguousarray(qkv, np.float32), sig=np.ascontiguousarray(sig, np.float32),
                span=np.asarray(span, np.int32))


def _signal(rng, B, T):
    sig = rng.standard_normal((B, T)).astype(np.float32)
    sig[sig == 0] = np.float32(1e-3)  # no accidental mask
    return sig


def _rng(*key):
    return np.random.default_rng([ord(c) for c in "/".join(map(str, key))])


SHAPES_T = (1, 31, 32, 33, 63, 64, 65, 96, 300, 512)
RAGGED_SPANS = ((1, 32, 33, 64), (65, 97, 481, 511))
RANGE_KINDS = ("scale1", "scale4", "rising", "falling", "creep")
GROUPS = ("shapes", "ragged", "masks", "range")


def _masks(T):
    """The six key-mask patterns of the masks group, [6, T] bool."""
    mk = np.zeros((6, T), bool)
    mk[0, 40] = True            # tile 1 alone: the upper half of wave 0's ballot
    mk[1, 70] = True            # tile 2 alone: the lower half of wave 1's ballot
    mk[2, :TILE] = True         # tile 0 wholly masked
    mk[3, :T - 1] = True        # one key left, the last
    mk[4, :] = True             # no key left: uniform over the span's keys
    mk[5, ::7] = True
    return mk


def _range_case(kind):
    B, T = 3, 512
    rng = _rng("range", kind)
    qkv = rng.standard_normal((B * T, 3 * D))
    if kind in ("rising", "falling"):
        # every query's scores grow (fall) along the keys: a rescale in most tiles (only in tile 0)
        ramp = np.linspace(0.0, 3.0, T) if kind == "rising" else np.linspace(3.0, 0.0, T)
        qkv[:, :D] = np.abs(qkv[:, :D]) * 0.5 + 1.0
        qkv[:, D:2 * D] = qkv[:, D:2 * D] * 0.2 + np.tile(ramp, B)[:, None]
    elif kind == "creep":
        # q ~ 1 in every dim: a score is 32 ramp(t) log2(e) / sqrt(32) log2 units; the ramp gives each tile of
        # 32 keys a maximum 7 above the tile before, under ENC_THR: a rescale every second tile, p up to 2^7
        per_key = 7.0 / TILE / (DH * math.log2(math.e) / math.sqrt(DH))
        qkv[:, :D] = 1.0 + 0.02 * qkv[:, :D]
        qkv[:, D:2 * D] = qkv[:, D:2 * D] * 0.02 + np.tile(np.arange(T) * per_key, B)[:, None]
    else:
        qkv *= {"scale1": 1.0, "scale4": 4.0}[kind]
    sig = _signal(rng, B, T)
    sig[0, ::7] = 0.0      # masked keys
    sig[2, :] = 0.0        # every key masked
    return _case(f"range {kind}", qkv, sig, [512, 300, 512])


@functools.lru_cache(maxsize=None)
def cases(group):
    """The cases of a group, built once per process (each seeded by its own name); a case is a dict of name,
    qkv [B * T, 768] f32, sig [B, T] f32, span [B] i32 (every span >= 1).  Callers must not modify the arrays."""
    out = []
    if group == "shapes":
        for T in SHAPES_T:
            rng = _rng(group, T)
            out.append(_case(f"shapes T={T}", rng.standard_normal((3 * T, 3 * D)), _signal(rng, 3, T),
                             [T, max(1, T // 2 + 1), 1]))
    elif group == "ragged":
        for spans in RAGGED_SPANS:
            rng = _rng(group, *spans)
            out.append(_case(f"ragged spans {spans}", rng.standard_normal((4 * 512, 3 * D)), _signal(rng, 4, 512),
                             spans))
    elif group == "masks":
        T, mk = 160, _masks(160)
        for i in (0, 3):
            rng = _rng(group, i)
            sig = _signal(rng, 3, T)
            sig[mk[i:i + 3]] = 0.0
            out.append(_case(f"masks patterns {i}..{i + 2}", rng.standard_normal((3 * T, 3 * D)), sig, [T] * 3))
    elif group == "range":
        out = [_range_case(kind) for kind in RANGE_KINDS]
    else:
        raise KeyError(group)
    return tuple(out)


def poisoned(case, value):
    """(qkv, sig) of a case with the qkv rows and samples at t >= span set to `value`."""
    B, T = case["sig"].shape
    dead = np.arange(T)[None, :] >= case["span"][:, None]
    qkv, sig = case["qkv"].reshape(B, T, 3 * D).copy(), case["sig"].copy()
    qkv[dead] = value
    sig[dead] = value
    return qkv.reshape(B * T, 3 * D), sig


PERSIST_SPANS = (64, 1, 33, 64, 17, 48)


@functools.lru_cache(maxsize=None)
def persistent_case(B):
    """T = 64, B chunks with spans cycling through PERSIST_SPANS; every fifth chunk all-masked, every third
    with one masked key."""
    T = 64
    rng = _rng("persistent", B)
    sig = _signal(rng, B, T)
    span = [PERSIST_SPANS[b % len(PERSIST_SPANS)] for b in range(B)]
    for b in range(B):
        if b % 5 == 0:
            sig[b, :] = 0.0
        elif b % 3 == 0:
            sig[b, (7 * b) % span[b]] = 0.0
    return _case(f"persistent B={B}", rng.standard_normal((B * T, 3 * D)), sig, span)


def sub_case(case, b):
    """Chunk b of a case as a case of its own (built once per case)."""
    subs = case.setdefault("_subs", {})
    if b not in subs:
        B, T = case["sig"].shape
        subs[b] = _case(f"{case['name']} chunk {b} span {case['span'][b]}", case["qkv"][b * T:(b + 1) * T],
                        case["sig"][b:b + 1], case["span"][b:b + 1])
    return subs[b]
