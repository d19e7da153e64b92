"""Float64 restatements behind tests/gpu_audio_check.py and tests/test_audio_host.py, and the inputs both use.

Resampler: torchaudio.functional.resample at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), the kernel in
float64 and rounded once to fp32: `dense_kernel` / `dense_resample` state it literally (F.pad + F.conv1d(stride=orig) in float64 on the
CPU); `band_of` / `banded_resample` state what the HIP kernel implements (per phase the first tap inside the window and Kb taps, the
products added in ascending tap order).  Trim: librosa.effects.trim in numpy, pad modes "constant" and "reflect".  Neither torchaudio
nor librosa is installed where these tests run, so parity with the libraries themselves is unpinned: these restatements are the reference."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
LPW, ROLLOFF = 6, 0.99
TILE = 1024                                      # outputs per workgroup of the resampler (ops.kernels_audio.TILE)
RATIOS = [(3, 1), (3, 2), (2, 3), (1, 2), (441, 320), (441, 160), (160, 441)]
AMIN = 1e-10


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def out_length(n, orig, new):
    return int(math.ceil(new * n / orig))


# ---------------------------------------------------------------------------------------------------------------------------
# resampler
# ---------------------------------------------------------------------------------------------------------------------------
def dense_kernel(orig, new, lpw=LPW, rolloff=ROLLOFF):
    """-> (t (new, 2 width + orig) float64 after the clamp, taps (new, 2 width + orig): float64 values of the fp32-rounded kernel, width)"""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=F64) / orig
    t = (torch.arange(0, -new, -1, dtype=F64)[:, None] / new + idx[None, :]) * base
    t = t.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    tp = t * math.pi
    taps = torch.where(tp == 0, torch.ones_like(tp), torch.sin(tp) / tp) * window * (base / orig)
    return t, taps.to(F32).to(F64), width


def dense_resample(x, orig, new, taps=None, width=None):
    """x (L) -> (ceil(new L / orig)) float64: torchaudio's _apply_sinc_resample_kernel, literally."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    if orig == new:
        return x.to(F64)
    if taps is None:
        _, taps, width = dense_kernel(orig, new)
    L = x.numel()
    xp = F.pad(x.to(F64).view(1, 1, L), (width, width + orig))
    y = F.conv1d(xp, taps.view(new, 1, -1), stride=orig)                  # (1, new, frames)
    return y.transpose(1, 2).reshape(-1)[:out_length(L, orig, new)]


def band_of(orig, new):
    """The banded table of the reduced pair: (band (Kb, new) float64 values of fp32 taps, 0 where a tap's |t| reached the clamp or lies
    beyond the dense kernel; first (new) ints; width; inside (new, 2 width + orig) bool)."""
    t, taps, width = dense_kernel(orig, new)
    inside = t.abs() < LPW
    first = [int(torch.nonzero(inside[p])[0]) for p in range(new)]
    Kb = max(int(inside[p].sum()) for p in range(new))
    band = torch.zeros(Kb, new, dtype=F64)
    for p in range(new):
        for k in range(Kb):
            j = first[p] + k
            if j < taps.shape[1] and bool(inside[p, j]):
                band[k, p] = taps[p, j]
    return band, first, width, inside


def banded_resample(x, orig, new, band, first, width, dtype=F64):
    """x (L) -> (ceil(new L / orig)) in `dtype`: y[q new + p] = sum_k band[k][p] x[q orig + first[p] + k - width], x = 0 outside [0, L),
    the products added in ascending k (one multiplication and one addition per tap in `dtype`)."""
    L, M = x.numel(), out_length(x.numel(), orig, new)
    Kb = band.shape[0]
    m = torch.arange(M)
    q, p = m // new, m % new
    start = q * orig + torch.as_tensor(first, dtype=torch.int64)[p] - width
    xd, bd = x.to(dtype), band.to(dtype)
    acc = torch.zeros(M, dtype=dtype)
    for k in range(Kb):
        i = start + k
        ok = (i >= 0) & (i < L)
        acc = acc + bd[k][p] * torch.where(ok, xd[i.clamp(0, max(L - 1, 0))] if L else torch.zeros(M, dtype=dtype), torch.zeros(M, dtype=dtype))
    return acc


def exact_lengths(orig, new, width):
    """The row lengths of the exact regime: 1, around width and orig, the lengths whose outputs end around one workgroup's TILE, and
    one where ceil(new L / orig) != floor."""
    want = [1, width - 1, width, width + 1, orig - 1, orig, orig + 1]
    for M in (TILE - 1, TILE, TILE + 1):
        want.append(next(L for L in range(1, 40000) if out_length(L, orig, new) >= M))       # the shortest row with at least M outputs
    if orig > 1:
        want.append(next(L for L in range(width + 2, 40000) if (new * L) % orig))             # ceil != floor
    return sorted({L for L in want if L >= 0})


def exact_case(orig, new, seed):
    """Integer taps and integer samples: every product and sum is exact in fp32, so the kernel must equal float64 exactly.
    -> (band (Kb, new) of integers in [-4, 4] at EVERY entry, first, width, rows: list of integer-valued fp32 vectors)"""
    band, first, width, _ = band_of(orig, new)
    g = gen(seed)
    iband = torch.randint(-4, 5, band.shape, generator=g).to(F64)
    rows = [torch.randint(-8, 9, (L,), generator=g).to(F32) for L in exact_lengths(orig, new, width)]
    return iband, first, width, rows


REAL_LENS = [9000, 4097, 2500, 333]


def real_rows(orig, new, seed):
    """A ragged batch of 4: seeded noise and chirps (0 -> 0.45 of the input rate), fp32."""
    g = gen(seed)
    rows = []
    for b, L in enumerate(REAL_LENS):
        if b % 2 == 0:
            rows.append((0.3 * torch.randn(L, generator=g)).to(F32))
        else:
            n = torch.arange(L, dtype=F64)
            rows.append((0.8 * torch.sin(math.pi * 0.45 * n * n / L)).to(F32))
    return rows


def resample_inputs():
    """Every resample input the GPU cases use: (orig, new, rows, kind)."""
    out = []
    for i, (orig, new) in enumerate(RATIOS):
        out.append((orig, new, exact_case(orig, new, 7100 + i)[3], "exact"))
        out.append((orig, new, real_rows(orig, new, 7200 + i), "real"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# trim
# ---------------------------------------------------------------------------------------------------------------------------
def frame_powers(y, frame_length, hop, pad_mode):
    """mean(x^2) of the 1 + L // hop centred frames of y (float64), the row padded with zeros or reflected."""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[0]
    left, right = frame_length // 2, frame_length - frame_length // 2
    if L == 0:
        padded = np.zeros(left + right)
    else:
        padded = np.pad(y, (left, right), mode=pad_mode)
    return np.array([np.mean(padded[i * hop:i * hop + frame_length] ** 2) for i in range(1 + L // hop)])


def frame_db(y, frame_length, hop, pad_mode):
    p = frame_powers(y, frame_length, hop, pad_mode)
    return 10.0 * np.log10(np.maximum(AMIN, p)) - 10.0 * np.log10(max(AMIN, p.max()))


def trim(y, top_db, frame_length, hop, pad_mode="constant"):
    """librosa.effects.trim -> (start, end); (0, 0) when no frame is non-silent."""
    loud = np.flatnonzero(frame_db(y, frame_length, hop, pad_mode) > -top_db)
    if loud.size == 0:
        return 0, 0
    return int(loud[0]) * hop, min(len(y), (int(loud[-1]) + 1) * hop)


def _burst(L, a, b, seed, amp=0.3, floor=1e-5):
    """floor-level noise with a burst of `amp`-level noise on [a, b)"""
    g = gen(seed)
    y = floor * torch.randn(L, generator=g)
    y[a:b] = amp * torch.randn(b - a, generator=g)
    return y.to(F32).numpy()


def trim_cases():
    """name -> dict(rows, top_db, frame_length, hop_length); every case runs under both pad modes."""
    c = {}
    fl, hop = 2048, 512
    # burst edges on frame boundaries (multiples of hop) and one sample either side of them
    c["burst_edges"] = dict(rows=[_burst(8192, 2048 + da, 5120 + db, 8100 + i) for i, (da, db) in
                                  enumerate([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)])], top_db=60, frame_length=fl, hop_length=hop)
    # hop does not divide L; L < frame_length; L < hop
    c["short_rows"] = dict(rows=[_burst(7001, 3000, 5000, 8110), _burst(1500, 600, 900, 8111), _burst(300, 100, 200, 8112)],
                           top_db=60, frame_length=fl, hop_length=hop)
    loud = _burst(6000, 1536, 4096, 8120)
    c["zeros_constant_loud_quiet"] = dict(rows=[np.zeros(5000, np.float32), np.full(4000, 0.5, np.float32), loud,
                                                (loud * np.float32(1e-4)).astype(np.float32)], top_db=60, frame_length=fl, hop_length=hop)
    c["top_db_0"] = dict(rows=[_burst(6000, 1536, 4096, 8130), np.full(3000, 0.25, np.float32)], top_db=0, frame_length=fl, hop_length=hop)
    c["frame_400_hop_160"] = dict(rows=[_burst(16000, 3200, 9600, 8140), _burst(9999, 1000, 1001, 8141), _burst(150, 20, 90, 8142)],
                                  top_db=40, frame_length=400, hop_length=160)
    c["odd_frame_401_hop_100"] = dict(rows=[_burst(5000, 1200, 3300, 8150), _burst(4100, 0, 50, 8151), _burst(401, 350, 401, 8152)],
                                      top_db=30, frame_length=401, hop_length=100)
    return c


PAD_MODES = ("constant", "reflect")
