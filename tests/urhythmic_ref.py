"""numpy restatement of the urhythmic segmentation search (reference urhythmic/segmenter.py: _segment, _backtrack, cluster_merge), the
inputs the fixture and the GPU cases share, and the CPU yardstick of the time stretcher.  Test infrastructure: the product never
imports it.

numba's typing of `_segment`, spelled out (under NumPy 2 a bare Python float is a weak scalar, so a literal transcription would compute
everything in float32 -- a different function):
  - D[t, s, :] = D[t, s - 1, :] + log_probs[s, :]      float32 + float32 -> float32, one rounding per step, in this order;
  - alpha[t - s] + D[t - s, t, k]                      float32 + float32 -> float32;
  - gamma * s                                          float64 (gamma float64 or int64, s int64);
  - (float32 sum) + (float64 product)                  float64;
  - alpha_max > alpha[t + 1]                           float64 against float64(float32);
  - alpha[t + 1] = alpha_max                           rounds to float32: the running maximum is held in float32.
The dense (T, T, K) table is not built: its row D[a, e, :] is a running sum carried along e."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "urhythmic_search.npz")
GOLDEN_STRETCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "urhythmic_stretch.npz")


# ---------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------
def span_scores(log_probs):
    """M[a, e] = max_k D[a, e, k], Kx[a, e] = argmax_k (numpy's: the smallest k), for a <= e."""
    lp = np.asarray(log_probs, np.float32)
    T = lp.shape[0]
    M = np.full((T, T), -np.inf, np.float32)
    Kx = np.zeros((T, T), np.int32)
    for a in range(T):
        r = lp[a].copy()
        M[a, a], Kx[a, a] = r.max(), r.argmax()
        for e in range(a + 1, T):
            r = r + lp[e]                                          # float32 arrays: a float32 sum
            M[a, e], Kx[a, e] = r.max(), r.argmax()
    return M, Kx


def search_tables(log_probs, gamma, rule="sequential"):
    """(alpha (T + 1,) float32, P (T + 1, 2) int32).  rule "sequential" is the reference's loop; "argmax" is the variant that takes
    the first float64 maximum of the candidates instead -- NOT the reference, kept to show that the inputs tell the two apart."""
    lp = np.asarray(log_probs, np.float32)
    T = lp.shape[0]
    M, Kx = span_scores(lp)
    g = np.float64(gamma)
    alpha = np.zeros(T + 1, np.float32)
    P = np.zeros((T + 1, 2), np.int32)
    for t in range(T):
        a = t - np.arange(t + 1)                                   # candidate s starts at frame t - s
        c = (alpha[a] + M[a, t]).astype(np.float64) + g * np.arange(t + 1).astype(np.float64)
        assert (alpha[a] + M[a, t]).dtype == np.float32 and c.dtype == np.float64
        if rule == "sequential":
            cur, best = np.float32(-np.inf), 0
            for s, cs in enumerate(c):
                if cs > np.float64(cur):
                    cur, best = np.float32(cs), s
        elif rule == "argmax":
            best = int(np.argmax(c))
            cur = np.float32(c[best])
        else:
            raise ValueError(rule)
        alpha[t + 1] = cur
        P[t + 1] = (t - best, Kx[t - best, t])
    return alpha, P


def backtrack(alpha, P):
    """(codes (T,) int32: the unit of every frame, boundaries (N + 1,) ascending from 0)"""
    rhs = len(alpha) - 1
    codes = np.zeros(rhs, np.int32)
    boundaries = [rhs]
    while rhs != 0:
        lhs, code = P[rhs]
        boundaries.append(int(lhs))
        codes[lhs:rhs] = code
        rhs = int(lhs)
    return codes, np.array(boundaries[::-1], np.int64)


def cluster_merge(labels, codes, boundaries):
    """codes (T,) per frame and boundaries (N + 1,) -> (clusters (M,), cluster boundaries (M + 1,))"""
    segments = codes[boundaries[:-1]]
    clusters = np.asarray(labels)[segments]
    opens = np.flatnonzero(np.diff(clusters, prepend=-1, append=-1))
    return clusters[opens[:-1]].astype(np.int32), np.asarray(boundaries)[opens].astype(np.int64)


def segment_all(log_probs, gamma, labels, rule="sequential"):
    """Everything the tests compare, as a dict of arrays."""
    alpha, P = search_tables(log_probs, gamma, rule)
    codes, boundaries = backtrack(alpha, P)
    if len(codes):
        clusters, cboundaries = cluster_merge(labels, codes, boundaries)
    else:
        clusters, cboundaries = np.zeros(0, np.int32), np.zeros(1, np.int64)
    return dict(alpha=alpha, P=P, codes=codes, boundaries=boundaries, clusters=clusters, cboundaries=cboundaries)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (shared by tools/gen_golden_urhythmic.py, the host tests and the GPU cases)
# ---------------------------------------------------------------------------------------------------------------------------
def default_labels(K):
    """A fixed unit -> cluster table with three clusters in runs of uneven length."""
    return ((np.arange(K) * 7 + 3) % 11 % 3).astype(np.int32)


def piecewise_log_probs(T, K, seed, sharp=4.0):
    """log_softmax of random logits with one dominant unit per stretch of 1 .. 11 frames."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, K))
    t = 0
    while t < T:
        n, k = int(rng.integers(1, 12)), int(rng.integers(0, K))
        logits[t:t + n, k] += sharp
        t += n
    z = logits - logits.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


ROUNDING_GAMMA = 0.7


def rounding_family(count=16, draws=20000):
    """T = 6, K = 2, lp = float32(-700 + 0.35 i), i uniform in -3 .. 3, gamma = 0.7: the first `count` draws of default_rng(0) on which
    the reference's rule and a plain float64 argmax choose different back-pointers."""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(draws):
        lp = (-700.0 + rng.integers(-3, 4, size=(6, 2)) * 0.35).astype(np.float32)
        if not np.array_equal(search_tables(lp, ROUNDING_GAMMA)[1], search_tables(lp, ROUNDING_GAMMA, "argmax")[1]):
            out.append(lp)
            if len(out) == count:
                break
    return out


def tie_inputs():
    """[(name, lp, gamma)]: exact ties over k (all equal; two identical dominant columns: the smaller k wins) and over s."""
    rng = np.random.default_rng(21)
    equal = np.full((20, 5), np.float32(np.log(0.2)), np.float32)
    twin = piecewise_log_probs(70, 6, seed=22)
    twin[:, 5] = twin[:, 2]                                       # two units with identical columns: wherever unit 2 wins, 5 ties with it
    flat = np.zeros((66, 3), np.float32)                          # gamma = 0: every candidate s of a frame has the same value
    steps = (-0.25 * rng.integers(1, 3, size=(40, 2))).astype(np.float32)   # quarter steps with gamma = 0.25: exact arithmetic, many ties
    return [("tie_all_equal", equal, 2.0), ("tie_twin_columns", twin, 2.0), ("tie_across_s_flat", flat, 0.0), ("tie_across_s_quarters", steps, 0.25)]


def fixture_inputs():
    """[(name, lp, gamma)] of the committed fixture: T <= 130, K <= 129."""
    out = [("piecewise_130x129_g2", piecewise_log_probs(130, 129, seed=1), 2.0),
           ("piecewise_65x100_g07", piecewise_log_probs(65, 100, seed=2, sharp=6.0), 0.7),
           ("piecewise_64x3_g2", piecewise_log_probs(64, 3, seed=3, sharp=2.0), 2.0),
           ("single_frame", piecewise_log_probs(1, 5, seed=4), 2.0)]
    out += [(f"rounding_{i:02d}", lp, ROUNDING_GAMMA) for i, lp in enumerate(rounding_family())]
    return out + tie_inputs()


def load_golden():
    """{name: dict(lp, gamma, labels, alpha, P, codes, boundaries, clusters, cboundaries)} from tests/golden/urhythmic_search.npz"""
    z = np.load(GOLDEN)
    out = {}
    for name in z["names"]:
        out[str(name)] = {k: z[f"{name}/{k}"] for k in ("lp", "gamma", "labels", "alpha", "P", "codes", "boundaries", "clusters", "cboundaries")}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the time stretcher: rhythm-model dictionaries of the fixture and the CPU yardstick
# ---------------------------------------------------------------------------------------------------------------------------
SOUND_TYPE_OF_CLUSTER = {0: "SONORANT", 1: "OBSTRUENT", 2: "SILENCE"}
# {sound type: (a, loc, scale)} as the reference's training script saves them; the target speaker is slower on sonorants, much faster
# on obstruents (some durations round to zero) and has longer silences
RHYTHM_SOURCE = {"SONORANT": (2.2, 0.0, 0.045), "OBSTRUENT": (2.9, 0.0, 0.030), "SILENCE": (1.4, 0.0, 0.120)}
RHYTHM_TARGET = {"SONORANT": (2.0, 0.0, 0.065), "OBSTRUENT": (1.1, 0.0, 0.004), "SILENCE": (1.5, 0.0, 0.150)}


def fixture_units(T, D=8, seed=31):
    return np.random.default_rng(seed).standard_normal((1, D, T)).astype(np.float32)


def interpolate_segments(units, plan, dtype):
    """units (D, T) torch CPU tensor; plan [(start, length, target)] -> (D, sum of targets): F.interpolate(mode="linear") per segment."""
    import torch
    import torch.nn.functional as F
    x = units.to(dtype)
    parts = [F.interpolate(x[None, :, s:s + n], mode="linear", size=d)[0] for s, n, d in plan]
    return torch.cat(parts, dim=-1) if parts else x[:, :0]
