"""Golden vectors for the pose discriminator, produced by EXECUTING the reference's own source (the reference tree is not part of this
repository, so the outputs are committed as a fixture):

  reference_disc_pose.npz   (results only; the fp32 inputs are tests/disc_cases.py: weights() and fixture_rows(), seeded)
                            src/discriminators.py (PoseDiscriminator.get_output) and src/ops.py (compute_loss_e_fake,
                            compute_loss_d_fake, compute_loss_d_real), unmodified, on the NumPy TensorFlow stand-in in float64
                            (oracle.tf_shim.install()).  What lines 998-1015 of compute_losses_prior (src/trainer_sequence_fc.py) do is
                            restated in `prior` below in this project's own words, because the trainer class itself needs a TF session, data loaders and a
                            config; the functions it calls are the reference's.

The ops the stand-in lacks (slim.flatten, tf.split, tf.reduce_sum, the `**` operator, slim.fully_connected under slim.arg_scope) are
added to the installed modules from this script with their documented TF semantics; oracle/ is not touched.

    python tests/golden/make_disc_golden.py <reference tree>        (or HMMR_REFERENCE_TREE)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HMMR_REFERENCE_TREE", "")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import disc_cases as D  # noqa: E402  (the fixture's seeded inputs live with the test that reads it)


def extend_shim(tf):
    T_, _a = tf.Tensor, tf._a

    def _axis(axis):
        return None if axis is None else tuple(int(a) for a in np.atleast_1d(_a(axis)))

    def reduce_sum(x, axis=None, keepdims=None, name=None, keep_dims=None):
        return T_(np.sum(_a(x), axis=_axis(axis), keepdims=bool(keepdims or keep_dims)))

    def split(value, num_or_size_splits, axis=0, num=None, name="split"):
        a = _a(value)
        assert isinstance(num_or_size_splits, int) and a.shape[axis] % num_or_size_splits == 0       # (an integer must divide the axis evenly)
        return [T_(p) for p in np.split(a, num_or_size_splits, axis=axis)]

    def flatten(inputs, outputs_collections=None, scope=None):
        a = _a(inputs)
        return T_(a.reshape(a.shape[0], -1))

    added = []
    for k, v in dict(reduce_sum=reduce_sum, split=split).items():
        assert not hasattr(tf, k), k
        setattr(tf, k, v)
        added.append((tf, k))
    slim = sys.modules["tensorflow.contrib.slim"]
    fc = tf.add_arg_scope(tf._fully_connected)                     # (slim.arg_scope takes decorated ops only)
    saved_fc = slim.fully_connected
    slim.fully_connected = fc
    slim.flatten = flatten
    had_pow = hasattr(T_, "__pow__")
    if not had_pow:
        T_.__pow__ = lambda self, o: T_(np.power(self.a, _a(o)))
    return added, (slim, saved_fc), had_pow


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        raise SystemExit("usage: make_disc_golden.py <reference tree> (a checkout of akanazawa/human_dynamics)")
    from oracle import tf_shim
    installed = tf_shim.install(np.float64)
    added, (slim, saved_fc), had_pow = extend_shim(tf_shim)
    import tensorflow as tf
    sys.path.insert(0, REF)
    try:
        from src.discriminators import PoseDiscriminator
        from src.ops import compute_loss_d_fake, compute_loss_d_real, compute_loss_e_fake
    finally:
        sys.path.remove(REF)
    Tn, _a = tf_shim.Tensor, tf_shim._a
    val = lambda x: np.asarray(_a(x), np.float64)
    tf_shim.WEIGHTS = {k: np.asarray(v, np.float64) for k, v in D.weights().items()}
    del tf_shim.USED_VARIABLES[:]
    eye = np.eye(3).reshape(1, 1, 9)
    full = lambda x: np.concatenate([np.tile(eye, (x.shape[0], 1, 1)), x.astype(np.float64)], axis=1).reshape(-1, 216)      # a global rotation in front
    real, fake = [full(x) for x in D.fixture_rows()]
    disc_pose = PoseDiscriminator(1e-4)

    def prior(rows_real, rows_fake):
        """what compute_losses_prior does with its rows, in this project's words: both segments of [n,24,9] rows end to end with a unit
        axis in front of the nine values, joint 0 left out, through the reference's get_output; the 24 outputs per row cut into the
        real and the fake half; the reference's three loss functions on the halves.  Equal counts, as the reference requires."""
        n = int(rows_real.shape[0])
        assert n == int(rows_fake.shape[0])
        both = tf.expand_dims(tf.concat([rows_real, rows_fake], 0), 2)
        scores = disc_pose.get_output(both[:, 1:])
        real_scores, fake_scores = tf.split(scores, 2)
        e, dr, df = compute_loss_e_fake(fake_scores), compute_loss_d_real(real_scores), compute_loss_d_fake(fake_scores)
        return scores, e, dr, df, df + dr

    out, e_pose, d_real, d_fake, d_pose = prior(Tn(real.reshape(-1, 24, 9)), Tn(fake.reshape(-1, 24, 9)))
    used = sorted(set(tf_shim.USED_VARIABLES))
    assert used == sorted(D.weights()), "the reference reads other variables than the bank packs"
    packed = dict(out=val(out), losses=np.array([float(val(e_pose)), float(val(d_real)), float(val(d_fake))]), d_pose=np.array(float(val(d_pose))),
                  inputs_sum=np.array([np.abs(real).sum(), np.abs(fake).sum(), sum(np.abs(v.astype(np.float64)).sum() for v in D.weights().values())]))
    assert packed["out"].shape == (sum(D.FIXTURE_ROWS), 24)
    path = os.path.join(HERE, "reference_disc_pose.npz")
    np.savez_compressed(path, **packed)
    print(path, os.path.getsize(path), sorted(packed), packed["losses"])
    for mod, k in added:
        delattr(mod, k)
    slim.fully_connected = saved_fc
    del slim.flatten
    if not had_pow:
        del tf_shim.Tensor.__pow__
    tf_shim.uninstall(installed)


if __name__ == "__main__":
    main()
