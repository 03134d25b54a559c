"""Shared by the fused-FFN tests (test_ffn_scheme.py on the CPU, test_gpu_ffn.py
on the GPU): the plain reference of the block csrc/ffn.hip computes, a numpy
model of the kernel's split-fp16 arithmetic, the bars both test files hold
results to, and the cases.

The block, from unfolded weights (encoder/transformer.py:36-54 with
position_ffn.py:27-40; the decoder's FFN is the middle line alone):

    yd  = y (+ att Wo^T + bo)                          the Wo fold in front
    x   = yd + W2 relu(W1 LN(yd) + b1) + b2
    qkv = LN_q(x) Wq^T + bq                            the next layer's fold behind

Forms: "none" (nd_op_enc_ffn), "wo" and "wo_qkv" (nd_op_enc_ffn_wo, in place),
"dec" (nd_op_dec_ffn: P16 rows, d_ff split over nsplit workgroups).

No GPU and nothing compiled is imported here.
"""
import functools
import math

import numpy as np
import torch

D, HC, BM, NQ = 256, 32, 128, 768
LN_EPS = 1e-6
F16_LIMIT = 65504.0
FORMS = ("none", "wo", "wo_qkv", "dec")
LO_TERMS = ("w_hi.a_lo", "w_lo.a_hi")

# The bar (test_ffn_scheme.py's docstring derives it): K is the smallest power of two for which the numpy
# model stays within a quarter of the bar on every case; fixed from the model alone.
K_BAR = 8.0
HALF_ULP = 2.0 ** -25


# ----------------------------------------------------------------- reference
def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (D,), g, b, LN_EPS)


def reference(case, wo, dtype=torch.float64):
    """(x [M, 256], qkv [M, 768], max hidden) of the block in `dtype` on the CPU.  float64 is the reference;
    float32 is the reference model's own arithmetic, whose error against float64 is the yardstick E32."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in case.items() if isinstance(v, np.ndarray)}
    yd = t["y"]
    if wo:
        yd = yd + t["att"] @ t["Wo"].t() + t["bo"]
    h = torch.relu(_ln(yd, t["lg"], t["lb"]) @ t["W1"].t() + t["b1"])
    x = yd + h @ t["W2"].t() + t["b2"]
    qkv = _ln(x, t["lq"], t["lqb"]) @ t["Wq"].t() + t["bq"]
    return x, qkv, float(h.max())


# ----------------------------------------------------------------- the shipped scheme
def split16(x):
    """fp32 x -> (hi, lo) as float64 arrays holding fp16 values: hi = fp16(x), lo = fp16(x - hi) (ff_split)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def weight_planes(W):
    """W f32 [N, K] -> (wh, wl, 2^s): launch_pack_p16h's power-of-two scale (max|W| 2^s in [2^13, 2^14)) and
    the hi / lo planes of W 2^s, as float64 arrays holding fp16 values."""
    W = np.asarray(W, np.float32)
    mx = float(np.abs(W).max())
    s = 2.0 ** (14 - int(np.frexp(mx)[1])) if mx > 0 and np.isfinite(mx) else 1.0
    wh, wl = split16(W * np.float32(s))
    return wh, wl, s


def fold_ln(W, b, g, beta):
    """launch_fold_layernorm: W' = W g in fp32, b' = b + W beta accumulated in fp64."""
    Wf = (W * g[None, :]).astype(np.float32)
    bf = (b.astype(np.float64) + W.astype(np.float64) @ beta.astype(np.float64)).astype(np.float32)
    return Wf, bf


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _accumulate(acc, ah, al, wh, wl, dropped=None):
    """One 32-wide k-block of a split-fp16 product into the fp32 accumulator acc [M, N]: the kernel's three
    MFMA terms in its order (w_hi a_lo, w_lo a_hi, w_hi a_hi), one fp32 rounding each (what the MFMA rounds
    inside a k-block is not modelled).  dropped: (term of LO_TERMS, column slice) left out."""
    with np.errstate(invalid="ignore", over="ignore"):
        for name, a, w in (("w_hi.a_lo", al, wh), ("w_lo.a_hi", ah, wl), (None, ah, wh)):
            term = a @ w.T
            if dropped is not None and dropped[0] == name:
                term[:, dropped[1]] = 0.0
            acc = _f32(acc.astype(np.float64) + term)
    return acc


def _product(acc, ah, al, wh, wl, drop, which):
    """acc [M, N] += a W^T over the 8 k-blocks of K = 256 (phase 1, the Wo fold, the QKV fold); drop =
    (which, slice j, term) leaves the term out of output columns 32 j .. 32 j + 31 on every k-block."""
    dropped = None
    if drop is not None and drop[0] == which:
        dropped = (drop[2], slice(HC * drop[1], HC * drop[1] + HC))
    for kb in range(D // 32):
        k = slice(32 * kb, 32 * kb + 32)
        acc = _accumulate(acc, ah[:, k], al[:, k], wh[:, k], wl[:, k], dropped)
    return acc


def _ln_f32(y):
    """The kernels' LayerNorm without affine: fp32, two-pass (the summation order is not modelled).
    Returns (LN(y), mean, M2)."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mu = (y.sum(axis=1, dtype=np.float32) * np.float32(1.0 / D)).astype(np.float32)
        d = y - mu[:, None]
        m2 = (d * d).sum(axis=1, dtype=np.float32)
        rs = (np.float32(1.0) / np.sqrt(m2 * np.float32(1.0 / D) + np.float32(LN_EPS))).astype(np.float32)
        return (d * rs[:, None]).astype(np.float32), mu, m2


def emulate(case, form, nsplit=1, drop=None, rows=None):
    """A numpy model of enc_ffn_kernel's arithmetic, written from the kernel's comments: dict of x [M, 256],
    mean [M], m2 [M] (the epilogue's row statistics) and, for "wo_qkv", qkv [M, 768], all float32.

    Activations (LN(y), the attention rows, the hidden, LN(x)) are split unscaled into fp16 hi + lo; the
    weights are folded and split at launch_pack_p16h's 2^s; a product is w_hi a_lo + w_lo a_hi + w_hi a_hi
    with one fp32 rounding per term and 32-wide k-block.  The accumulators start at (y + b2) 2^s (with the Wo
    fold at (x + bo) 2^s_o, whose result is rescaled, LayerNorm'd and restarted as (yd + b2) 2^s) and walk the
    d_ff chunks of 32 hidden units in order; "dec" walks split sp's chunks sp nall / nsplit ..
    (sp + 1) nall / nsplit - 1 from 0 (split 0 from the residual and b2) and sums the partials in split order.
    The QKV fold runs from the epilogue's fp32 x and its statistics.

    drop = (which, j, term): term of LO_TERMS left out of ONE chunk: which = "W1" / "W2": d_ff chunk j (phase 1
    of its 32 hidden units / its phase-2 k-block); "Wo" / "Wq": output slice j of 32 columns.
    rows: a row index (slice or array) to model a subset; a row's result does not depend on the others.
    """
    rows = slice(None) if rows is None else rows
    y = case["y"][rows]
    F = case["W1"].shape[0]
    nall = F // HC
    wo, dec = form in ("wo", "wo_qkv"), form == "dec"
    W1f, b1f = fold_ln(case["W1"], case["b1"], case["lg"], case["lb"])
    w1h, w1l, s1 = weight_planes(W1f)
    w2h, w2l, s2 = weight_planes(case["W2"])
    with np.errstate(invalid="ignore", over="ignore"):
        if wo:
            woh, wol, so = weight_planes(case["Wo"])
            ah, al = split16(case["att"][rows])
            acc = _f32((y + case["bo"][None, :]).astype(np.float32).astype(np.float64) * so)
            acc = _product(acc, ah, al, woh, wol, drop, "Wo")
            y = _f32(acc.astype(np.float64) / so)
        ln, _, _ = _ln_f32(y)
        lh, ll = split16(ln)
        init = _f32((y + case["b2"][None, :]).astype(np.float32).astype(np.float64) * s2)
        # phase 1 of every chunk (a chunk's hidden units depend on no other chunk)
        hacc = _product(np.zeros((y.shape[0], F), np.float32), lh, ll, w1h, w1l, drop, "W1")
        h = np.maximum(_f32(_f32(hacc.astype(np.float64) / s1).astype(np.float64) + b1f[None, :]), np.float32(0))
        hh, hl = split16(h)
        ns = nsplit if dec else 1
        parts = []
        for sp in range(ns):
            acc = init if sp == 0 else np.zeros_like(init)
            for j in range(sp * nall // ns, (sp + 1) * nall // ns):
                k = slice(HC * j, HC * j + HC)
                dropped = (drop[2], slice(None)) if drop is not None and drop[0] == "W2" and drop[1] == j else None
                acc = _accumulate(acc, hh[:, k], hl[:, k], w2h[:, k], w2l[:, k], dropped)
            parts.append(acc)
        if ns > 1:
            acc = np.zeros_like(init)
            for p in parts:
                acc = _f32(acc.astype(np.float64) + p)
        x = _f32(acc.astype(np.float64) / s2)
        lnx, mean, m2 = _ln_f32(x)
        out = dict(x=x, mean=mean, m2=m2, hmax=float(np.nanmax(h)) if h.size else 0.0)
        if form == "wo_qkv":
            Wqf, bqf = fold_ln(case["Wq"], case["bq"], case["lq"], case["lqb"])
            qh, ql, sq = weight_planes(Wqf)
            xh, xl = split16(lnx)
            qacc = _product(np.zeros((x.shape[0], NQ), np.float32), xh, xl, qh, ql, drop, "Wq")
            out["qkv"] = _f32(_f32(qacc.astype(np.float64) / sq).astype(np.float64) + bqf[None, :])
    return out


# ----------------------------------------------------------------- the bars
def n_acc(F, form, nsplit=1):
    """The roundings the residual-carrying accumulator takes, from the scheme's description: three per d_ff
    chunk of 32; 24 more with the Wo fold (8 k-blocks of three terms); the decoder form: split 0's share of
    the chunks, plus the nsplit additions of the sum in split order."""
    nall = F // HC
    if form == "dec":
        return 3 * (nall // nsplit) + (nsplit if nsplit > 1 else 0)
    return 3 * nall + (24 if form in ("wo", "wo_qkv") else 0)


def yardsticks(case, wo):
    """dict of a case's references with or without the Wo fold, computed once: x, qkv (fp64 numpy), e32,
    e32q (max error of the fp32 block against them), mx, mxq (max |ref|), hidden (max hidden unit).  Kept in
    the case dict under a private "_ref" key (like test_gpu_ffn.py's "_dev" device copies): these caches
    are the one exception to "callers must not modify" a case; the arrays of a case are never written."""
    key = "_ref_wo" if wo else "_ref"
    if key not in case:
        x, q, hid = reference(case, wo)
        x32, q32, _ = reference(case, wo, torch.float32)
        x, q = x.numpy(), q.numpy()
        case[key] = dict(x=x, qkv=q, e32=float(np.abs(x32.numpy().astype(np.float64) - x).max()),
                         e32q=float(np.abs(q32.numpy().astype(np.float64) - q).max()),
                         mx=float(np.abs(x).max()), mxq=float(np.abs(q).max()), hidden=hid)
    return case[key]


def acc_term(case, form, which="x", nsplit=1):
    """The accumulation term of the bar, the same formula for either output: a random walk of n_acc half-ulp
    roundings at the output's max|ref| (max|x_ref| for "x", max|qkv_ref| for "qkv")."""
    ys = yardsticks(case, form in ("wo", "wo_qkv"))
    walk = math.sqrt(n_acc(case["W1"].shape[0], form, nsplit)) * HALF_ULP
    return walk * (ys["mx"] if which == "x" else ys["mxq"])


def bars(case, form, which="x", nsplit=1):
    """(K (E32 + the accumulation term), the old ceiling 2e-4 max(1, max|ref| / 8)) of output `which`
    ("x" or "qkv") of a case in a form."""
    ys = yardsticks(case, form in ("wo", "wo_qkv"))
    e32, mx = (ys["e32"], ys["mx"]) if which == "x" else (ys["e32q"], ys["mxq"])
    return K_BAR * (e32 + acc_term(case, form, which, nsplit)), 2e-4 * max(1.0, mx / 8.0)


def error(case, form, got, which="x", rows=None):
    """max |got - fp64| of output `which` (over `rows` of the case when the model ran on a subset)."""
    ref = yardsticks(case, form in ("wo", "wo_qkv"))[which]
    ref = ref if rows is None else ref[rows]
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


def stats_miss(x, mean, m2):
    """The row statistics against fp64 statistics of the returned fp32 x itself: (worst |mean - mean64| over its
    bar 2^-22 max|x_row|, worst |M2 - M2_64| over its bar 1e-5 M2_64 + 256 (2^-23 max|x_row|)^2).  Both <= 1
    when the statistics hold."""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1)
    q = ((x - mu[:, None]) ** 2).sum(axis=1)
    top = np.abs(x).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rm = np.abs(np.asarray(mean, np.float64) - mu) / np.maximum(2.0 ** -22 * top, np.finfo(np.float64).tiny)
        rq = np.abs(np.asarray(m2, np.float64) - q) / np.maximum(1e-5 * q + 256.0 * (2.0 ** -23 * top) ** 2,
                                                                 np.finfo(np.float64).tiny)
    return float(np.nan_to_num(rm, nan=np.inf).max()), float(np.nan_to_num(rq, nan=np.inf).max())


def one_pass_stats(x):
    """The mistake the statistics bar must catch: mean and M2 = sum x^2 - 256 mean^2 in one fp32 pass."""
    x = np.asarray(x, np.float32)
    mean = (x.sum(axis=1, dtype=np.float32) * np.float32(1.0 / D)).astype(np.float32)
    sq = (x * x).sum(axis=1, dtype=np.float32)
    return mean, (sq - np.float32(D) * mean * mean).astype(np.float32)


# ----------------------------------------------------------------- cases
def _rng(*key):
    return np.random.default_rng([ord(c) for c in "/".join(map(str, key))])


def _weights(rng, F):
    n = lambda *s: rng.standard_normal(s)
    return dict(W1=n(F, D) / 16, b1=0.1 * n(F), W2=n(D, F) / math.sqrt(F), b2=0.1 * n(D), lg=1 + 0.1 * n(D),
                lb=0.1 * n(D), Wo=n(D, D) / 16, bo=0.1 * n(D), Wq=n(NQ, D) / 16, bq=0.1 * n(NQ), lq=1 + 0.1 * n(D),
                lqb=0.1 * n(D))


def _case(name, group, y, att, w):
    M = y.shape[0]
    F = w["W1"].shape[0]
    assert y.shape == (M, D) and att.shape == (M, D) and F % HC == 0 and HC <= F <= 2048, name
    c = dict(name=name, group=group, M=M, F=F, y=np.ascontiguousarray(y, np.float32),
             att=np.ascontiguousarray(att, np.float32))
    c.update({k: np.ascontiguousarray(v, np.float32) for k, v in w.items()})
    return c


SHAPES_M = (1, 15, 16, 17, 127, 128, 129, 131, 272)
SHAPES_F = (32, 64, 96, 160, 2048)
# every M and every F; F = 32 and F = 2048 also at the 48 rows the CPU model's teeth use
UNIT_SHAPES = ((1, 32), (15, 64), (16, 96), (17, 160), (127, 2048), (128, 32), (129, 96), (131, 160), (272, 2048),
               (131, 64), (48, 2048), (48, 32), (272, 96))
GROUPS = ("unit", "residual", "offset", "small", "sparse", "outlier")
MODEL_ROWS_AT_2048 = 48
CONST = 100.0     # the constant rows: every partial sum of up to 256 of them is exact in fp32, in any order


def model_rows(case):
    """The rows the CPU model runs of a case: all, or 48 spread over the case at F = 2048."""
    if case["F"] < 2048 or case["M"] <= MODEL_ROWS_AT_2048:
        return None
    return np.unique(np.linspace(0, case["M"] - 1, MODEL_ROWS_AT_2048).astype(np.int64))


def _unit(rng, M):
    return rng.standard_normal((M, D)) * 2 + 0.5


@functools.lru_cache(maxsize=None)
def unit_case(M, F):
    """y ~ N(0.5, 2), att ~ N(0, 1) and the plain weights at M rows and d_ff F (seeded by M and F)."""
    rng = _rng("unit", "N(0.5,2)", M, F)
    w = _weights(rng, F)
    return _case(f"unit N(0.5,2) M={M} F={F}", "unit", _unit(rng, M), rng.standard_normal((M, D)), w)


@functools.lru_cache(maxsize=None)
def cases(group):
    """The cases of a group, built once per process (each seeded by its own name).  A case is a dict of name,
    group, M, F, y and att [M, 256] and the unfolded weights W1 [F, 256], b1, W2 [256, F], b2, lg, lb (the
    FFN's LayerNorm), Wo, bo, Wq [768, 256], bq, lq, lqb (the next layer's), all float32.  Callers must not
    modify the arrays; the only entries added to a case are the private caches "_ref", "_ref_wo" (yardsticks)
    and "_dev" (test_gpu_ffn.py), computed once from the unchanged arrays."""
    out = []

    def add(name, M, F, y_of, att_scale=1.0, edit=None):
        rng = _rng(group, name, M, F)
        w = _weights(rng, F)
        y = y_of(rng, M)
        att = rng.standard_normal((M, D)) * att_scale
        if edit is not None:
            edit(rng, w)
        out.append(_case(f"{group} {name} M={M} F={F}", group, y, att, w))

    if group == "unit":
        out = [unit_case(M, F) for M, F in UNIT_SHAPES]
    elif group == "residual":
        add("scale 64", 131, 2048, lambda r, M: r.standard_normal((M, D)) * 64)
        add("scale 1024", 48, 2048, lambda r, M: r.standard_normal((M, D)) * 1024)

        def mixed(r, M):   # rows of scale 1, 64, 1024 and 2^-7 side by side in one 128-row block
            return r.standard_normal((M, D)) * np.array([1.0, 64.0, 1024.0, 2.0 ** -7])[np.arange(M) % 4][:, None]
        add("mixed 1 | 64 | 1024 | 2^-7", 128, 96, mixed)
    elif group == "offset":
        def grid(r, M):
            # mean 100, std 1e-2, on a grid of 2^-9: every fp32 partial sum of a row (< 2^15) and so its mean
            # are exact in any order.  Off the grid the mean of such a row is good to half an ulp of 100 at
            # best, 3.8e-6, which LN turns into 4e-4 of every LN(y) element and 2e-3 of x: a kernel (or the
            # model) whose sum runs in another order could then miss the 2.6e-3 ceiling for no fault of the
            # algorithm.  On the grid the kernel and the model are exact in y - mean and what is left is the
            # algorithm: two passes, the variance of the differences.  The grid does not help E32: torch's
            # fp32 layer_norm loses the same 2e-3 on these rows, so without the Wo fold ("none", "dec") the x
            # bar of this case is the 2.6e-3 ceiling, far above what the kernel gives (4e-5), and a dropped
            # term would not show there.  The case's teeth are the statistics, the constant rows and the Wo
            # forms (yd of std 1: E32 3.5e-5); dropped terms are for the unit cases to catch.
            y = 100.0 + np.round(1e-2 * r.standard_normal((M, D)) * 512.0) / 512.0
            y[[0, 5, M - 1]] = CONST
            return y
        add("mean 100 std 1e-2", 129, 64, grid)
    elif group == "small":
        # y small: the LayerNorm restores scale 1 before W1.  Under the Wo fold the attention rows stay at
        # scale 1 (yd is then att Wo^T + bo); the third case is the other way round, attention rows whose lo
        # parts are fp16 subnormals under a residual of scale 1.  (Attention rows AND residual at 2^-14 are
        # left out: the split of att then keeps ~11 bits, test_split_fp16_scheme.py's subnormal regime, and
        # the LayerNorm behind the residual turns that into 5e-5 of x in the model, 330 E32.)
        add("scale 2^-7", 127, 160, lambda r, M: r.standard_normal((M, D)) * 2.0 ** -7)
        add("scale 2^-14", 16, 32, lambda r, M: r.standard_normal((M, D)) * 2.0 ** -14)
        add("att 2^-14 under N(0.5,2)", 17, 96, _unit, 2.0 ** -14)
    elif group == "sparse":
        def dead(r, w):     # W1 LN(y) ~ N(0, 1): about 0.6 % of the hidden units survive b1 = -2.5
            w["b1"] = w["b1"] - 2.5

        def wide(r, w):     # hidden units from ~1e-4 to ~1e3: rows of W1 (and b1) scaled by 10^U(-4, 3)
            sc = 10.0 ** r.uniform(-4.0, 3.0, w["W1"].shape[0])
            w["W1"] = w["W1"] * sc[:, None]
            w["b1"] = w["b1"] * sc
        add("b1 = -2.5", 131, 160, _unit, edit=dead)
        add("hidden 1e-4 .. 1e3", 17, 2048, _unit, edit=wide)
        add("hidden 1e-4 .. 1e3", 129, 96, _unit, edit=wide)
    elif group == "outlier":
        def one_big(r, w):  # one weight of each matrix a thousand times its typical size
            for k in ("W1", "W2", "Wo", "Wq"):
                W = w[k]
                i, j = int(r.integers(W.shape[0])), int(r.integers(W.shape[1]))
                W[i, j] = 1000.0 * float(np.sqrt((W ** 2).mean())) * (1 if W[i, j] >= 0 else -1)
        add("one weight x1000", 127, 64, _unit, edit=one_big)
        add("one weight x1000", 16, 2048, _unit, edit=one_big)
    else:
        raise KeyError(group)
    return tuple(out)


def all_cases():
    return [c for g in GROUPS for c in cases(g)]


def sub_case(case, rows, name):
    """Rows of a case as a case of its own (weights shared, not copied)."""
    c = {k: v for k, v in case.items() if not k.startswith("_")}
    c.update(name=f"{case['name']} {name}", y=np.ascontiguousarray(case["y"][rows]),
             att=np.ascontiguousarray(case["att"][rows]))
    c["M"] = c["y"].shape[0]
    return c
