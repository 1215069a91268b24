"""hmmr_adam_step (csrc/adam.hip) on the device against the float32 NumPy restatement of TF's ApplyAdam (tests/adam_cases.py): p, m and v
are required to equal the oracle's BYTES after steps 1, 2, 3 and 12 -- the file is compiled without contraction and with the IEEE
division and square root, so there is no tolerance to choose.  Every segment lies inside one buffer between guard floats, at float
offsets 0 .. 3 from a 16-byte boundary (the 16-byte path needs all four pointers aligned: each is misaligned on its own too); lengths
around the 16-byte piece, the wave and the kernel's 4096-value chunk; 1, 2, 64 and 65 segments in one call (65 crosses the launch
boundary).  Denormal behaviour is not asserted: every value of the cases is a normal float32 or an exact zero
(test_adam_cases.py::test_oracle_intermediates_stay_normal)."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as A
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
GF = A.GUARD_FLOATS


class _Arena(object):
    """one int32 device buffer filled with the guard pattern; `place(values, offset)` puts an array at float offset `offset` past the
    next 16-byte boundary with guard floats on both sides and returns its (start, length) in floats"""

    def __init__(self, floats, device):
        self.host = np.full(floats, A.GUARD, np.int32)
        self.device, self.used, self.dev = device, 0, None
        self.spans = []

    def place(self, values, offset):
        start = (self.used + GF + 3) // 4 * 4 + offset
        n = len(values)
        assert start + n + GF <= len(self.host)
        self.host[start:start + n] = np.asarray(values, np.float32).view(np.int32)
        self.used = start + n
        self.spans.append((start, n))
        return start, n

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(self.device)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, span):
        return self.dev.data_ptr() + 4 * span[0]

    def read(self, span):
        return self.dev[span[0]:span[0] + span[1]].cpu().numpy().view(np.float32)

    def guards_untouched(self):
        got = self.dev.cpu().numpy()
        mask = np.ones(len(got), bool)
        for s, n in self.spans:
            mask[s:s + n] = False
        return bool((got[mask] == A.GUARD).all())


def _hyper(k):
    return L.AdamHyper(A.LR, A.BETA1, A.BETA2, A.EPS, float(A.powers(A.BETA1, k)), float(A.powers(A.BETA2, k)))


def _call(lib, table, n, k):
    L.check(lib.hmmr_adam_step(table, n, C.byref(_hyper(k)), torch.cuda.current_stream().cuda_stream), "hmmr_adam_step")


class _Problem(object):
    """segments (length, (offset of p, g, m, v), gradient kind) in one arena; `run` makes 12 steps and compares at CHECK_STEPS"""

    def __init__(self, specs, device, seed=0, null_g=(), per_segment_calls=False):
        self.specs, self.null_g, self.per_segment_calls = specs, set(null_g), per_segment_calls
        total = sum(4 * (n + GF + 8) for n, _, _ in specs) + 64
        self.arena = _Arena(total, device)
        self.p0 = [A.values(n, seed + i) for i, (n, _, _) in enumerate(specs)]
        self.sp, self.sg, self.sm, self.sv = [], [], [], []
        for i, (n, off, kind) in enumerate(specs):
            self.sp.append(self.arena.place(self.p0[i], off[0]))
            self.sg.append(self.arena.place(np.zeros(n, np.float32), off[1]))
            self.sm.append(self.arena.place(np.zeros(n, np.float32), off[2]))
            self.sv.append(self.arena.place(np.zeros(n, np.float32), off[3]))
        self.arena.upload()
        self.seed = seed

    def grad(self, i, k):
        n, _, kind = self.specs[i]
        return A.gradients(kind, n, k, seed=self.seed + 7 * i)

    def table(self):
        t = (L.AdamSeg * len(self.specs))()
        for i, (n, _, _) in enumerate(self.specs):
            t[i].p, t[i].m, t[i].v, t[i].n = self.arena.ptr(self.sp[i]), self.arena.ptr(self.sm[i]), self.arena.ptr(self.sv[i]), n
            t[i].g = None if i in self.null_g else self.arena.ptr(self.sg[i])
        return t

    def run(self, steps=12):
        lib, ar = L.load(), self.arena
        table = self.table()
        ref = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in self.p0]
        for k in range(steps):
            for i, span in enumerate(self.sg):
                g = self.grad(i, k)
                ar.dev[span[0]:span[0] + span[1]] = torch.from_numpy(g.view(np.int32)).to(ar.device)
                if i not in self.null_g and span[1] > 0:
                    ref[i] = A.step32(ref[i][0], g, ref[i][1], ref[i][2], A.powers(A.BETA1, k), A.powers(A.BETA2, k))
            if self.per_segment_calls:
                for i in range(len(self.specs)):
                    _call(lib, C.cast(C.byref(table, i * C.sizeof(L.AdamSeg)), C.POINTER(L.AdamSeg)), 1, k)
            else:
                _call(lib, table, len(self.specs), k)
            if k + 1 in A.CHECK_STEPS:
                torch.cuda.synchronize()
                for i in range(len(self.specs)):
                    for name, span, want in (("p", self.sp[i], ref[i][0]), ("m", self.sm[i], ref[i][1]), ("v", self.sv[i], ref[i][2])):
                        got = ar.read(span)
                        assert got.tobytes() == want.tobytes(), ("step %d segment %d %s (n=%d, offsets %s): %d values differ, first at %s"
                                                                 % (k + 1, i, name, self.specs[i][0], self.specs[i][1],
                                                                    int((got.view(np.int32) != want.view(np.int32)).sum()),
                                                                    np.flatnonzero(got.view(np.int32) != want.view(np.int32))[:4]))
                assert ar.guards_untouched(), "step %d: a guard float was written" % (k + 1)
        return ref


PLACEMENTS = [(o, o, o, o) for o in A.OFFSETS] + [tuple(o if j == i else 0 for j in range(4)) for i in range(4) for o in (1, 2, 3)]


@pytest.mark.parametrize("offsets", PLACEMENTS, ids=["p%d_g%d_m%d_v%d" % o for o in PLACEMENTS])
def test_every_length_at_every_placement_matches_the_oracle_bytes(offsets, gpu_device):
    """all nine lengths in one call, each placed with `offsets`; mixed magnitudes with exact zeros among them"""
    specs = [(n, offsets, "some_zeros" if i % 2 else "mixed") for i, n in enumerate(A.LENGTHS)]
    _Problem(specs, gpu_device, seed=sum(offsets)).run()


@pytest.mark.parametrize("count", A.SEGMENT_COUNTS)
def test_segment_counts_across_the_launch_boundary(count, gpu_device):
    """1, 2, 64 and 65 segments in one call, lengths and placements cycling; some without a gradient or empty: they keep their bytes"""
    specs = [(A.LENGTHS[i % len(A.LENGTHS)] if i % 11 != 5 else 0, PLACEMENTS[i % len(PLACEMENTS)], "mixed") for i in range(count)]
    null_g = [i for i in range(count) if i % 7 == 3]
    prob = _Problem(specs, gpu_device, seed=count, null_g=null_g)
    prob.run()
    for i in null_g:                                   # p as placed, m and v still zero
        assert prob.arena.read(prob.sp[i]).tobytes() == prob.p0[i].tobytes()
        assert not prob.arena.read(prob.sm[i]).view(np.int32).any() and not prob.arena.read(prob.sv[i]).view(np.int32).any()


def test_one_call_of_65_segments_equals_65_calls_of_one(gpu_device):
    specs = [(A.LENGTHS[i % len(A.LENGTHS)], PLACEMENTS[(3 * i) % len(PLACEMENTS)], "mixed") for i in range(65)]
    a, b = _Problem(specs, gpu_device, seed=65), _Problem(specs, gpu_device, seed=65, per_segment_calls=True)
    a.run(steps=3)
    b.run(steps=3)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.dev, b.arena.dev)


def test_zero_gradients_leave_every_byte(gpu_device):
    """exact zero gradients on zero moments: p, m and v keep exactly their values, at both paths"""
    specs = [(n, off, "zeros") for n in (5, 64, 4097) for off in ((0, 0, 0, 0), (1, 0, 0, 0))]
    prob = _Problem(specs, gpu_device, seed=3)
    before = prob.arena.dev.clone()
    prob.run(steps=3)
    assert torch.equal(prob.arena.dev, before)


def test_elements_do_not_depend_on_the_segmentation(gpu_device):
    """one tensor of 9001 values as one segment, and cut into 7 segments at odd places: the same bytes (and the same twice)"""
    n, cuts = 9001, (0, 1, 6, 70, 1093, 5190, 5193, 9001)
    p0 = A.values(n, 11)
    g = [A.gradients("mixed", n, k, seed=5) for k in range(3)]
    lib = L.load()
    results = []
    for pieces in ((0, n), cuts, cuts):
        bufs = [torch.from_numpy(x.copy()).to(gpu_device) for x in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32))]
        for k in range(3):
            gd = torch.from_numpy(g[k]).to(gpu_device)
            t = (L.AdamSeg * (len(pieces) - 1))()
            for i, (a, b) in enumerate(zip(pieces[:-1], pieces[1:])):
                t[i].p, t[i].g, t[i].m, t[i].v, t[i].n = bufs[0].data_ptr() + 4 * a, gd.data_ptr() + 4 * a, bufs[1].data_ptr() + 4 * a, bufs[2].data_ptr() + 4 * a, b - a
            _call(lib, t, len(pieces) - 1, k)
        torch.cuda.synchronize()
        results.append([b.cpu().numpy() for b in bufs])
    ref = A.run32(p0, g)[-1]
    for r in results:
        for got, want in zip(r, ref):
            assert got.tobytes() == want.tobytes()


def test_tfadam_steps_tensors_and_advances_its_powers(gpu_device):
    """optim.TFAdam over three tensors, one of them without a gradient: the oracle's bytes after 3 steps, float32 power products"""
    from human_dynamics_amd.engine import HmmrEngine
    from human_dynamics_amd.optim import TFAdam
    eng = HmmrEngine(None, None, device=gpu_device)
    shapes = ((3, 5), (85,), (64, 65))
    p0 = [A.values(int(np.prod(s)), 20 + i).reshape(s) for i, s in enumerate(shapes)]
    ts = [torch.from_numpy(p.copy()).to(gpu_device).requires_grad_() for p in p0]
    opt = TFAdam(eng, ts, lr=A.LR, beta1=A.BETA1, beta2=A.BETA2, epsilon=A.EPS)
    ref = [(p.reshape(-1), np.zeros(p.size, np.float32), np.zeros(p.size, np.float32)) for p in p0]
    for k in range(3):
        assert opt.beta1_power == A.powers(A.BETA1, k) and opt.beta2_power == A.powers(A.BETA2, k)
        for i, t in enumerate(ts):
            if i == 1 and k == 1:
                t.grad = None                          # a step without a gradient for this variable
                continue
            g = A.gradients("mixed", t.numel(), k, seed=30 + i)
            t.grad = torch.from_numpy(g).to(gpu_device).reshape(t.shape)
            ref[i] = A.step32(ref[i][0], g, ref[i][1], ref[i][2], A.powers(A.BETA1, k), A.powers(A.BETA2, k))
        opt.step()
        opt.zero_grad()
        assert all(t.grad is None for t in ts)
    for i, t in enumerate(ts):
        for got, want in zip((t.detach(), opt.m[i], opt.v[i]), ref[i]):
            assert got.cpu().numpy().reshape(-1).tobytes() == want.tobytes()
