"""numpy restatement of the stretch-plan kernel's contract (s2svc_useg_plan in include/s2svc_hip.h), the rhythm model of the fixture and
the random segment rows the host test and the GPU cases share.  Test infrastructure: the product never imports it.
tests/test_rhythm_table_host.py pins plan_rows to the host code that ships (rhythm model -> stretch_plan -> segment_table)."""
import numpy as np

import urhythmic_ref as UR
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.urhythmic import rhythm_model as RM
from seq2seq_vc_amd.urhythmic.rhythm_model import SHORT_SILENCE

SOUND = {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}
SONORANT_ID, OBSTRUENT_ID, SILENCE_ID = 0, 1, 2
INT32_MAX = 2**31 - 1


def rhythm_model(source=None, target=None):
    rm = U.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in (source or UR.RHYTHM_SOURCE).items()},
                        "target": {getattr(U, n): v for n, v in (target or UR.RHYTHM_TARGET).items()}})
    return rm


def plan_rows(clusters, cboundaries, ncl, table, silence_cluster, short_silence=SHORT_SILENCE):
    """clusters (B, Tmax), cboundaries (B, Tmax + 1), ncl (B), table (n_clusters, Lmax + 1), all integer arrays ->
    (seg (B, Tmax, 4), nsegs (B), totals (B), status (B)) int32.  Entries at or beyond ncl[b] are never looked at."""
    clusters, cboundaries, table = np.asarray(clusters), np.asarray(cboundaries), np.asarray(table)
    B, Tmax = clusters.shape
    n_clusters, Lmax = table.shape[0], table.shape[1] - 1
    seg = np.zeros((B, Tmax, 4), np.int32)
    nsegs, totals, status = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        rows, off, bad, unmapped = [], 0, False, False
        for i in range(min(max(int(ncl[b]), 0), Tmax)):
            lo, hi, c = int(cboundaries[b, i]), int(cboundaries[b, i + 1]), int(clusters[b, i])
            n = hi - lo
            if not (0 <= lo <= Tmax and 0 <= hi <= Tmax and 1 <= n <= Lmax and 0 <= c < n_clusters):
                bad = True
                continue
            if c == silence_cluster and n <= short_silence:
                continue
            target = int(table[c, n])
            if target == RM.UNMAPPED:
                unmapped = True
            elif target > 0:
                rows.append((lo, n, target, off))
                off += target                                      # a Python int: no overflow
        status[b] = 2 if bad else 1 if unmapped else 3 if off > INT32_MAX else 0
        if status[b] == 0:
            seg[b, :len(rows)] = np.array(rows, np.int64).reshape(-1, 4)
            nsegs[b], totals[b] = len(rows), off
    return seg, nsegs, totals, status


def random_row(rng, nseg, max_len=12, edge=False):
    """(cluster ids, boundaries): nseg segments, no two neighbours of the same cluster; `edge`: lengths drawn from the edge cases
    (silences of exactly 3 and 4 frames, obstruents of 1 .. 8 frames: the fixture's target maps <= 7 to zero frames)."""
    clusters, bounds = [], [0]
    for _ in range(nseg):
        c = int(rng.choice([k for k in (SONORANT_ID, OBSTRUENT_ID, SILENCE_ID) if not clusters or k != clusters[-1]]))
        if edge and c == SILENCE_ID:
            n = int(rng.choice([3, 4]))
        elif edge and c == OBSTRUENT_ID:
            n = int(rng.integers(1, 9))
        else:
            n = int(rng.integers(1, max_len + 1))
        clusters.append(c)
        bounds.append(bounds[-1] + n)
    return clusters, bounds


def pack_rows(rows, Tmax, fill=(0, 0)):
    """[(cluster ids, boundaries)] -> clusters (B, Tmax), cboundaries (B, Tmax + 1), ncl (B) int32; entries past a row's own hold `fill`
    = (what clusters holds there, what cboundaries holds there)."""
    B = len(rows)
    clusters, cboundaries = np.full((B, Tmax), fill[0], np.int32), np.full((B, Tmax + 1), fill[1], np.int32)
    for b, (cl, cb) in enumerate(rows):
        clusters[b, :len(cl)] = cl
        cboundaries[b, :len(cb)] = cb
    return clusters, cboundaries, np.array([len(cl) for cl, _ in rows], np.int32)
