"""The ragged sliding-window rule of include/hmmr_hip.h (hmmr_predict_tracks) restated in NumPy, and the offset lists the tests of the
plan (tests/test_tracks_plan.py, which pins this restatement to the reference's recorded windows) and of the two device copies
(tests/test_gpu_tracks_call.py) share."""
import numpy as np

T, FOV, MARGIN, G = 20, 13, 6, 8
# no track; only empty ones; empty tracks in front of, between and behind tracks of 1, g - 1, g, g + 1, T and more frames; 130 tracks, so
# that the 65th and the 129th start a new 64-track chunk of the kernels' argument table
LENGTHS = {"none": [], "all_empty": [0, 0, 0], "mixed": [1, 0, 7, 8, 9, 0, 20, 33, 0], "many": [(1, 0, 9)[i % 3] for i in range(130)]}


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=off[1:])
    return off


def ragged_rule(off, T=T, margin=MARGIN, g=G):
    """fed [n_windows][T]: the global frame in every slot (-1: the zero image); owner [n_windows]: (track, local window); kept: per
    window the (slot, output row) pairs"""
    fed, owner, kept = [], [], []
    for k in range(len(off) - 1):
        n_k = int(off[k + 1] - off[k])
        for lw in range(-(-n_k // g)):
            f = lw * g + np.arange(T) - margin
            fed.append(np.where((f >= 0) & (f < n_k), off[k] + f, -1))
            owner.append((k, lw))
            kept.append([(margin + j, int(off[k]) + lw * g + j) for j in range(min(g, n_k - lw * g))])
    return np.array(fed, np.int64).reshape(-1, T), owner, kept
