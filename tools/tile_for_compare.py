#!/usr/bin/env python3
"""HmmrEngine._tile_for of another revision against this tree's (hmmr_conv_tile_for, csrc/conv_tiles.h), point by point; no GPU.

    git show REV:human_dynamics_amd/engine.py > /tmp/engine_rev.py
    python tools/tile_for_compare.py /tmp/engine_rev.py

Every combination of k_order {0, 1, 2} x layer name x the three operand dtypes (and None) x 11 values of cout x candidates 0 .. 40.
Prints the number of points; exit status 1 when any differs."""
import importlib.util
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from human_dynamics_amd import _lib as L          # noqa: E402
from human_dynamics_amd import engine as E        # noqa: E402

spec = importlib.util.spec_from_file_location("human_dynamics_amd._engine_other", sys.argv[1])
other = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = other
spec.loader.exec_module(other)                    # (its relative imports are this package's)

COUTS = (8, 64, 72, 128, 192, 256, 320, 512, 1024, 1280, 2048)
points, bad = 0, []
for k_order, nm, dt, cout, cand in itertools.product((0, 1, 2), ("shortcut", "conv1", "conv2", "conv3"), (L.HMMR_F32, L.HMMR_BF16, L.HMMR_F16X3, None),
                                                     COUTS, range(41)):
    lay = L.Layer()
    lay.k_order = k_order
    was, now = other.HmmrEngine._tile_for(lay, cand, cout, dt, nm), E.HmmrEngine._tile_for(lay, cand, cout, dt, nm)
    points += 1
    if was != now:
        bad.append((k_order, nm, dt, cout, cand, was, now))
for b in bad[:20]:
    print("k_order %d %s dtype %s cout %d candidate %d: was %d, is %d" % b)
print("_tile_for: %d points, %d differ" % (points, len(bad)))
sys.exit(1 if bad else 0)
