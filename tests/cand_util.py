"""Candidate scoring (test code): the candidates the tests build from a fixture gold row, the padded
[B, K, L] arrays a call takes, and the scripted score rows of the posterior tests."""
import numpy as np

KINDS = ("gold", "substitution", "deletion", "first")


def candidates_of(g, n_special=4, vocab=8):
    """The four candidates of a gold row ``g`` (tokens without EOS, at least one): g itself, g with its middle
    token replaced by the next base token, g with its middle token deleted, and g[:1]."""
    g = [int(t) for t in g]
    mid = len(g) // 2
    sub = list(g)
    sub[mid] = n_special + (g[mid] - n_special + 1) % (vocab - n_special)
    return [g, sub, g[:mid] + g[mid + 1:], g[:1]]


def pack(cands, K, L, pad_idx, eos_idx):
    """cand [B, K, L] int32 (tokens, EOS, then pad_idx) and cand_len [B, K] (EOS counted, 0 = empty slot) of
    ``cands``: per chunk a list of at most K id lists."""
    cand = np.full((len(cands), K, L), pad_idx, np.int32)
    cand_len = np.zeros((len(cands), K), np.int32)
    for b, cl in enumerate(cands):
        for k, t in enumerate(cl):
            cand[b, k, : len(t)] = t
            cand[b, k, len(t)] = eos_idx
            cand_len[b, k] = len(t) + 1
    return cand, cand_len


def scripted_rows():
    """(scores [5, 4] f32, cand_len [5, 4] i32, best [5]): a two-way tie (the lowest slot wins), a row with
    every slot empty, a K-of-1 row, a row near -400 whose scores differ by 1e-3, and a row with a NaN."""
    scores = np.array([[-3.0, -1.5, -1.5, -7.0],
                       [-2.0, -3.0, -4.0, -5.0],
                       [-9.0, -12.5, 5.0, 0.0],
                       [-400.0, -400.001, -399.999, -400.002],
                       [-1.0, np.nan, -2.0, -0.5]], np.float32)
    cand_len = np.array([[3, 4, 4, 2], [0, 0, 0, 0], [0, 5, 0, 0], [7, 7, 9, 7], [2, 2, 2, 0]], np.int32)
    return scores, cand_len, np.array([1, -1, 1, 2, 0])


def logsumexp_posterior(scores, cand_len):
    """A direct fp64 log-softmax over the non-empty slots, written without the module under test."""
    s = np.asarray(scores, np.float64)
    post = np.full(s.shape, -np.inf)
    for b in range(s.shape[0]):
        live = np.flatnonzero(np.asarray(cand_len)[b] > 0)
        if len(live):
            v = s[b, live]
            post[b, live] = v - (v.max() + np.log(np.exp(v - v.max()).sum()))
    return post
