"""References and cases for the BiLSTM recurrence (lstm_dir_kernel, csrc/lstm.hip), CPU only.

One NanoEncoder layer with the packing semantics of encoder/nano_encoder.py
(pack_padded_sequence, nn.LSTM(bidirectional), pad_packed_sequence, eval
BatchNorm): gates in i, f, g, o order; sequence b runs only its steps
t < len[b]; the reverse direction starts at len[b] - 1; rows t >= len[b] are
zero; the BatchNorm touches valid rows only.  Layer 0 forms its projections
from a scalar sample (signal * wih0 + bsum), the other layers read them (xp).

- bilstm(case): the layer in numpy, fp64 by default.
- yardstick(case): the same layer in fp32 on the CPU: torch.nn.LSTM over the
  packed inputs (enforce_sorted=False), or bilstm(dtype=float32) where torch
  refuses a length of 0.
- case(name) / refs(name): the GPU suite's cases (tests/test_gpu_lstm.py) and,
  computed once, each one's fp64 reference, E32 = max |fp32 - fp64| and the
  floor 2^-23 max |ref|, one fp32 rounding of the output.

Every input is built in fp32 and widened, so both references and the kernel
see identical numbers.
"""
import functools

import numpy as np

H, G = 128, 512
F32 = np.float32


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def projections(c, dtype=np.float64):
    """Per direction [B, T, 512]: x W_ih^T + b_ih + b_hh as the layer sees it."""
    B, T = c["B"], c["T"]
    if c.get("xp") is not None:
        xp = c["xp"].astype(dtype).reshape(B, T, 2, G)
        return [xp[:, :, 0], xp[:, :, 1]]
    s = c["signal"].astype(dtype)[:, :, None]
    return [s * c["wih0"][d].astype(dtype) + c["bsum"][d].astype(dtype) for d in range(2)]


def bilstm(c, dtype=np.float64, recurrent=None, sigmoid=_sigmoid, tanh=np.tanh, gate_sum=None):
    """out [B, T, 256] (fwd | bwd), zeros at t >= len.  recurrent(d, h) -> [B, 512]
    replaces h W_hh[d]^T and gate_sum(x, z) the sum x + z (tests/test_lstm_scheme.py
    restates the kernel's arithmetic through them)."""
    B, T, lens = c["B"], c["T"], c["lens"].astype(np.int64)
    out = np.zeros((B, T, 2 * H), dtype)
    proj = projections(c, dtype)
    rows = np.arange(B)
    for d in range(2):
        Wt = c["whh"][d].astype(dtype).T
        h, cell = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        for step in range(int(lens.max(initial=0))):
            act = step < lens
            pos = np.where(act, step if d == 0 else lens - 1 - step, 0)
            x = proj[d][rows, pos]
            z = recurrent(d, h) if recurrent else h @ Wt
            z = gate_sum(x, z) if gate_sum else x + z
            i, f, o = sigmoid(z[:, :H]), sigmoid(z[:, H:2 * H]), sigmoid(z[:, 3 * H:])
            g = tanh(z[:, 2 * H:3 * H])
            c2 = (f * cell + i * g).astype(dtype)
            h2 = (o * tanh(c2)).astype(dtype)
            cell = np.where(act[:, None], c2, cell)
            h = np.where(act[:, None], h2, h)
            out[rows[act], pos[act], d * H:(d + 1) * H] = h2[act]
    return batchnorm(c, out, dtype)


def batchnorm(c, out, dtype):
    if c.get("bn_scale") is None:
        return out
    valid = valid_rows(c)
    sc, sh = c["bn_scale"].astype(dtype).reshape(-1), c["bn_shift"].astype(dtype).reshape(-1)
    return np.where(valid[:, :, None], (out * sc).astype(dtype) + sh, out).astype(dtype)


def valid_rows(c):
    return np.arange(c["T"])[None, :] < c["lens"][:, None]


def yardstick(c):
    """The layer in fp32 on the CPU, [B, T, 256] float32."""
    if (c["lens"] < 1).any():
        return bilstm(c, F32)
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    B, T = c["B"], c["T"]
    layer0 = c.get("xp") is None
    lstm = torch.nn.LSTM(1 if layer0 else 2 * G, H, bidirectional=True, batch_first=True)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            getattr(lstm, "weight_hh_l0" + sfx).copy_(torch.from_numpy(c["whh"][d].copy()))
            getattr(lstm, "bias_hh_l0" + sfx).zero_()
            if layer0:
                wih, bih = c["wih0"][d][:, None], c["bsum"][d]
            else:  # direction d reads its own 512 projections: a 0 / 1 matrix, exact in fp32
                wih, bih = np.zeros((G, 2 * G), F32), np.zeros(G, F32)
                wih[:, d * G:(d + 1) * G] = np.eye(G, dtype=F32)
            getattr(lstm, "weight_ih_l0" + sfx).copy_(torch.from_numpy(np.array(wih)))
            getattr(lstm, "bias_ih_l0" + sfx).copy_(torch.from_numpy(np.array(bih)))
        x = torch.from_numpy((c["signal"].reshape(B, T, 1) if layer0 else c["xp"].reshape(B, T, 2 * G)).copy())
        lens = torch.from_numpy(c["lens"].astype(np.int64))
        y, _ = lstm(pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(y, batch_first=True, total_length=T)
    return batchnorm(c, y.numpy(), F32)


# ----------------------------------------------------------------- cases
def make(B, T, lens, layer0, bn, seed, wmag=0.15):
    """Unit-scale projections, W_hh uniform in +-wmag; the inputs past each
    length are as random as the rest (a kernel that reads them shows)."""
    rng = np.random.default_rng(seed)
    c = dict(B=B, T=T, lens=np.asarray(lens, np.int32), xp=None, bn_scale=None, bn_shift=None,
             whh=rng.uniform(-wmag, wmag, (2, G, H)).astype(F32))
    assert c["lens"].shape == (B,) and c["lens"].max() <= T and c["lens"].min() >= 0
    if layer0:
        c["signal"] = rng.standard_normal((B, T)).astype(F32)
        c["wih0"] = rng.standard_normal((2, G)).astype(F32)
        c["bsum"] = (0.5 * rng.standard_normal((2, G))).astype(F32)
    else:
        c["xp"] = rng.standard_normal((B * T, 2 * G)).astype(F32)
    if bn:  # distinct per direction and unit, either sign
        c["bn_scale"] = (rng.uniform(0.5, 1.5, (2, H)) * rng.choice([-1.0, 1.0], (2, H))).astype(F32)
        c["bn_shift"] = rng.standard_normal((2, H)).astype(F32)
    return c


def _ragged(B, T, seed):
    """B distinct lengths in 1..T, unsorted, T among them but not in slot 0."""
    rng = np.random.default_rng(1000 + seed)
    lens = list(rng.choice(np.arange(1, T), B - 1, replace=False))
    lens.insert(1 + (B - 1) // 2, T)
    return lens


def _group(B, layer0, bn):
    return lambda: make(B, 40, _ragged(B, 40, B), layer0, bn, seed=B)


def _edit(build, fn):
    def f():
        c = build()
        fn(c)
        return c
    return f


def _one_weight(value, rest=0.1):
    def fn(c):  # one entry per direction carries max |W|
        c["whh"] = (c["whh"] * F32(rest / 0.15)).astype(F32)
        c["whh"][0, 200, 17] = value
        c["whh"][1, 77, 101] = -value
    return fn


def _tiny_whh(c):
    """max |W_hh| = 2^-120, the other entries 0 or smaller"""
    rng = np.random.default_rng(5)
    w = np.zeros((2, G, H), F32)
    idx = rng.integers(0, G * H, 300)
    w.reshape(2, -1)[:, idx] = F32(2.0 ** -122) * rng.uniform(-1, 1, (2, 300)).astype(F32)
    w[0, 3, 5] = w[1, 400, 99] = F32(2.0 ** -120)
    c["whh"] = w


def _saturate(mag):
    def fn(c):  # +-mag on each gate in turn (gate = t % 4, sign by t / 4), every other unit
        xp = c["xp"].reshape(c["B"], c["T"], 2, 4, H)
        for t in range(c["T"]):
            xp[:, t, :, t % 4, (t // 8) % 2::2] = mag if (t // 4) % 2 == 0 else -mag
    return fn


def _open_cell(c):
    """i, f, g wide open: c grows by ~1 a step to ~T, tanh(c) saturates"""
    xp = c["xp"].reshape(c["B"], c["T"], 2, 4, H)
    xp[:, :, :, 0:3, :] = 20.0


def _dir_scales(c):
    c["whh"][1] = (c["whh"][1] / F32(64)).astype(F32)


_BASE0 = lambda: make(4, 24, [24, 9, 17, 20], False, False, seed=40)  # noqa: E731  (W_hh = 0 and the tiny W_hh share it)

# name: (builder, discriminating).  Shapes are the smallest that reach the path: 4 sequences per workgroup in the
# split form (a full group runs the FULL loop, a partly filled one the guarded loop), 16 in the fp32 form.
CASES = {
    # grouping: unsorted distinct lengths, T 40
    "group_B4": (_group(4, True, False), True),
    "group_B5": (_group(5, False, True), True),
    "group_B7": (_group(7, False, False), True),
    "group_B8": (_group(8, True, True), True),
    "group_B6": (_group(6, False, False), True),
    "group_B16": (_group(16, True, False), True),
    "group_B17": (_group(17, False, True), True),
    "group_B33": (_group(33, False, False), True),
    # length edges, one group each
    "T1": (lambda: make(3, 1, [1, 1, 1], True, True, seed=20), False),
    "all_len_1": (lambda: make(4, 6, [1, 1, 1, 1], False, True, seed=21), False),
    "maxlen_odd": (lambda: make(4, 50, [31, 47, 12, 46], False, False, seed=22), False),
    "maxlen_even": (lambda: make(4, 50, [31, 46, 12, 45], True, False, seed=23), False),
    "T_1_0_Tm1": (lambda: make(4, 24, [24, 1, 0, 23], False, True, seed=24), False),
    "zero_group": (lambda: make(20, 18, [0] * 16 + [9, 17, 3, 12], True, True, seed=25), False),
    "short_slot0": (lambda: make(4, 30, [2, 30, 29, 17], False, False, seed=26), False),
    # long recurrence
    "long_512": (lambda: make(5, 512, [512, 511, 300, 1, 512], False, False, seed=30), True),
    # weight scale
    "wmax_2^1": (_edit(lambda: make(4, 24, [24, 9, 17, 20], False, False, seed=41), _one_weight(F32(2.0))), False),
    "wmax_2^-3": (_edit(lambda: make(5, 24, [24, 9, 17, 20, 3], True, False, seed=42), _one_weight(F32(0.125))), False),
    "one_weight_40x": (_edit(lambda: make(4, 24, [13, 24, 17, 20], False, True, seed=43),
                             _one_weight(F32(2.4), rest=0.06)), False),
    "dir0_64x_dir1": (_edit(lambda: make(6, 24, [24, 9, 17, 20, 5, 11], False, False, seed=44, wmag=0.4),
                            _dir_scales), False),
    "whh_zero": (_edit(_BASE0, lambda c: c["whh"].fill(0)), False),
    "whh_tiny": (_edit(_BASE0, _tiny_whh), False),
    # saturation
    "sat_20": (_edit(lambda: make(4, 16, [16, 9, 16, 13], False, False, seed=50), _saturate(20.0)), False),
    "sat_50": (_edit(lambda: make(4, 16, [16, 9, 16, 13], False, False, seed=51), _saturate(50.0)), False),
    "sat_90": (_edit(lambda: make(5, 16, [16, 9, 16, 13, 7], False, True, seed=52), _saturate(90.0)), False),
    "sat_200": (_edit(lambda: make(4, 16, [16, 9, 16, 13], False, False, seed=53), _saturate(200.0)), False),
    "open_cell": (_edit(lambda: make(4, 40, [40, 9, 33, 39], False, False, seed=54), _open_cell), False),
    # BatchNorm on valid rows only, both input forms
    "bn_layer0": (lambda: make(6, 21, [21, 4, 20, 13, 1, 8], True, True, seed=60), False),
    "bn_xp": (lambda: make(9, 21, [6, 21, 20, 13, 1, 8, 2, 19, 5], False, True, seed=61), False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name][0]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def refs(name):
    """(ref fp64 [B, T, 256], E32, floor) of a case; computed once, read-only."""
    c = case(name)
    ref = bilstm(c)
    ref.setflags(write=False)
    valid = valid_rows(c)
    e32 = float(np.abs(yardstick(c).astype(np.float64) - ref)[valid].max())
    floor = 2.0 ** -23 * float(np.abs(ref[valid]).max())
    return ref, e32, floor


FACTOR = {"f32": 4.0, "split": 8.0}  # the bars in force (the BiLSTM recurrence's error table)


def bar(name, form):
    _, e32, floor = refs(name)
    return FACTOR[form] * max(e32, floor)


def _small_h():
    """Output gate nearly closed (h ~ 1e-4) under W_hh entries up to 16: entered unscaled, h's lo part would sit
    in the fp16 subnormals (tests/test_lstm_scheme.py: without the 2^10 the scheme misses this case's bar)."""
    c = make(4, 24, [24, 9, 17, 20], False, False, seed=70, wmag=16.0)
    xp = c["xp"].reshape(4, 24, 2, 4, H)
    xp[:, :, :, 3, :] = -9.2 + 0.1 * xp[:, :, :, 3, :]
    return c


CASES["small_h"] = (_small_h, False)
