"""hmmr_strip_mse (csrc/losses.hip; the trainer's e_hallucinate) and its Python routes (HmmrEngine.strip_mse, ops.mean_squared_error)
against torch in float64: the loss and both gradients within FACTOR = 4 x E32, E32 being |the same computation in float32 - float64|
on the host (floored, for the one-number loss ALONE, at half a unit in the last place of a float32 of its size: the closest a float32 result
can be promised to lie).  Rows carry padded leading dimensions between guard floats; d_b == -d_a bytewise; a NULL output is never
written.  With `-s` every case prints its errors and E32."""
import numpy as np
import pytest
import torch

from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
FACTOR = 4.0
GUARD = 0x7FC12345
SHAPES = ((1, 1), (1, 2048), (3, 7), (10, 2048), (40, 2048))      # (rows, cols): one value, one row, odd and small, (2, 5) and (8, 5) strips
_ENGINE = {}


def _engine(device):
    if device not in _ENGINE:
        from human_dynamics_amd.engine import HmmrEngine
        _ENGINE[device] = HmmrEngine(None, None, device=device)
    return _ENGINE[device]


def _inputs(rows, cols):
    rng = np.random.default_rng([rows, cols, 17])
    return rng.standard_normal((rows, cols)).astype(np.float32), (0.5 * rng.standard_normal((rows, cols)) + 0.1).astype(np.float32)


def _reference(a, b, dtype, weight=1.0):
    ta, tb = (torch.from_numpy(x).to(dtype).requires_grad_() for x in (a, b))
    loss = torch.nn.functional.mse_loss(tb, ta)                   # mean over all elements
    (loss * weight).backward()
    return float(loss.detach()), ta.grad.double().numpy(), tb.grad.double().numpy()


def _bounds(a, b, weight=1.0):
    l64, da64, db64 = _reference(a, b, torch.float64, weight)
    l32, da32, db32 = _reference(a, b, torch.float32, weight)
    half_unit = 0.5 * float(np.spacing(np.float32(abs(l64))))
    # (the gradients take the raw E32: no floor)
    return (l64, da64, db64), (FACTOR * max(abs(l32 - l64), half_unit), FACTOR * float(np.abs(da32 - da64).max()), FACTOR * float(np.abs(db32 - db64).max()))


def _padded(x, ld, device):
    """rows of x at row stride ld inside a guard-filled buffer -> (buffer, the [rows, cols] view)"""
    rows, cols = x.shape
    buf = torch.full((rows * ld + 16,), GUARD, dtype=torch.int32, device=device)
    view = buf[8:8 + rows * ld].view(torch.float32).view(rows, ld)[:, :cols]
    view.copy_(torch.from_numpy(x).to(device))
    return buf, view


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("pad", (0, 3))
def test_loss_and_gradients_match_float64(rows, cols, pad, gpu_device):
    eng, lib = _engine(gpu_device), L.load()
    a, b = _inputs(rows, cols)
    weight = 1.0 if pad == 0 else 0.375
    (l64, da64, db64), (bl, bda, bdb) = _bounds(a, b, weight)
    lda, ldb, ld_da, ld_db = cols + pad, cols + 2 * pad, cols + pad, cols + 3 * pad
    abuf, av = _padded(a, lda, gpu_device)
    bbuf, bv = _padded(b, ldb, gpu_device)
    dabuf, dav = _padded(np.zeros_like(a), ld_da, gpu_device)
    dbbuf, dbv = _padded(np.zeros_like(a), ld_db, gpu_device)
    loss = torch.full((3,), GUARD, dtype=torch.int32, device=gpu_device)
    nbytes = lib.hmmr_strip_mse_workspace_bytes(rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream

    def call(want_loss=True, want_a=True, want_b=True):
        L.check(lib.hmmr_strip_mse(av.data_ptr(), lda, bv.data_ptr(), ldb, rows, cols, weight, loss.data_ptr() + 4 if want_loss else None,
                                   dav.data_ptr() if want_a else None, ld_da, dbv.data_ptr() if want_b else None, ld_db, ws.data_ptr(), nbytes, stream),
                "hmmr_strip_mse")
        torch.cuda.synchronize()

    call()
    got_l = float(loss.view(torch.float32)[1])
    got_da, got_db = dav.cpu().numpy(), dbv.cpu().numpy()
    e = (abs(got_l - l64), float(np.abs(got_da - da64).max()), float(np.abs(got_db - db64).max()))
    print("strip_mse %2d x %4d pad %d: loss err %.2e (E32 %.2e)  d_a err %.2e (E32 %.2e)  d_b err %.2e (E32 %.2e)"
          % (rows, cols, pad, e[0], bl / FACTOR, e[1], bda / FACTOR, e[2], bdb / FACTOR))
    assert e[0] <= bl and e[1] <= bda and e[2] <= bdb, (e, (bl, bda, bdb))
    assert (-got_da).tobytes() == got_db.tobytes()                                      # d_b == -d_a bytewise
    # guards: the loss's neighbours, the padding columns of every buffer, the inputs themselves
    assert int(loss[0]) == GUARD and int(loss[2]) == GUARD
    for buf, ld in ((dabuf, ld_da), (dbbuf, ld_db)):
        body = buf[8:8 + rows * ld].view(rows, ld)
        assert bool((buf[:8] == GUARD).all()) and bool((buf[8 + rows * ld:] == GUARD).all()) and bool((body[:, cols:] == GUARD).all())
    assert torch.equal(av.cpu(), torch.from_numpy(a)) and torch.equal(bv.cpu(), torch.from_numpy(b))
    # the same inputs give the same bytes; a NULL output is never written
    first = (loss.clone(), dabuf.clone(), dbbuf.clone())
    call()
    assert torch.equal(loss, first[0]) and torch.equal(dabuf, first[1]) and torch.equal(dbbuf, first[2])
    for skip in range(3):
        for t in (loss, dabuf, dbbuf):
            t.fill_(GUARD)
        call(*[i != skip for i in range(3)])
        for i, (t, ref) in enumerate(zip((loss, dabuf, dbbuf), first)):
            if i == skip:
                assert bool((t == GUARD).all()), "output %d was NULL and was written" % i
            else:
                assert torch.equal(t, ref)


def test_autograd_reaches_both_arguments(gpu_device):
    from human_dynamics_amd import ops
    eng = _engine(gpu_device)
    a, b = _inputs(10, 2048)
    (l64, da64, db64), (bl, bda, bdb) = _bounds(a, b, 3.0)
    ta = torch.from_numpy(a).to(gpu_device).reshape(2, 5, 2048).requires_grad_()
    tb = torch.from_numpy(b).to(gpu_device).reshape(2, 5, 2048).requires_grad_()
    loss = ops.mean_squared_error(ta, tb, engine=eng)
    assert loss.dim() == 0 and abs(float(loss.detach()) - l64) <= bl
    (3.0 * loss).backward()
    assert float(np.abs(ta.grad.cpu().numpy().reshape(10, 2048) - da64).max()) <= bda
    assert float(np.abs(tb.grad.cpu().numpy().reshape(10, 2048) - db64).max()) <= bdb
    # one side only: the other gets no gradient and its cotangent is not computed
    ta.grad = tb.grad = None
    ops.mean_squared_error(ta.detach(), tb, engine=eng).backward()
    assert ta.grad is None and float(np.abs(tb.grad.cpu().numpy().reshape(10, 2048) * 3.0 - db64).max()) <= bdb
    with pytest.raises(ValueError):
        ops.mean_squared_error(ta, tb[:, :4], engine=eng)
