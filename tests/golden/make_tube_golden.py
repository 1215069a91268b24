"""Golden vectors for the tube augmentor, produced by EXECUTING the reference's own source here
(/root/reference is not on the GPU box, so the outputs are committed as a fixture):

  reference_tube.npz   src/util/tube_augmentation.py `TubePreprocessor.__call__` and everything it calls in
                       src/util/data_utils.py (bounded_random_walk, jitter_center, jitter_scale, pad_image_edge,
                       rotate_img, flip_image, reflect_pose, reflect_joints3d, rescale_image) and src/tf_smpl/batch_lbs.py
                       (batch_rodrigues, batch_rot2aa), unmodified, on the NumPy TensorFlow stand-in in float32
                       (oracle.tf_shim.install(np.float32)).

The elementary ops the stand-in lacks (map_fn, cond, fill, less, random_uniform, cumsum, abs, slice, reverse, to_int32,
to_float, transpose, where, acos, sqrt, trace, clip_by_value, size, subtract, multiply, the `**` / `%` / `<=` operators of its
Tensor, and Python scalars kept weakly typed in its arithmetic operators so that a float32 run stays float32) are added to the installed module from this script with their documented TF semantics.  TWO ops are NOT the
reference's code and NOT TensorFlow's binary: `tf.image.resize_images` and `tf.contrib.image.rotate` are
tests/tube_oracle.py's `tf_resize_bilinear` and `tf_rotate_bilinear`, restatements of the published TF 1.8 kernels (as
make_reference_golden.py says of cv2.resize).  Everything else that shapes the fixture -- the walks, the integers, the
pad and the slice, the labels, poses and joints -- is the reference's own code.  `random_uniform` draws from a seeded NumPy
generator and records its draws: TensorFlow's random stream cannot be reproduced, only what the reference does with it.
TubePreprocessorDriver is a placeholder / Session.run wrapper around this call plus a transpose of [T,25,3] labels;
the preprocessor is called directly with [T,3,25] labels.

    python tests/golden/make_tube_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DRAWS = []
RNG = [None]


def extend_shim(tf, O):
    T, _a = tf.Tensor, tf._a

    def _w(o):
        """a Python scalar stays one: TF gives it the tensor's dtype, NumPy keeps the array's only for a scalar (not for the
        0-d float64 array the stand-in's own operators make of it, which would carry float64 through a float32 run)"""
        return o if isinstance(o, (int, float)) and not isinstance(o, bool) else _a(o)
    T._bin = lambda self, o, f: T(f(self.a, _w(o)))
    T.__radd__ = lambda self, o: T(np.add(_w(o), self.a))
    T.__rsub__ = lambda self, o: T(np.subtract(_w(o), self.a))
    T.__rmul__ = lambda self, o: T(np.multiply(_w(o), self.a))
    T.__rtruediv__ = lambda self, o: T(np.divide(_w(o), self.a))
    T.__rpow__ = lambda self, o: T(np.power(_w(o), self.a))
    T.__mod__ = lambda self, o: T(np.mod(self.a, _w(o)))          # tf.floormod: the sign of the divisor, like np.mod
    T.__le__ = lambda self, o: T(np.less_equal(self.a, _w(o)))
    T.__bool__ = lambda self: bool(self.a)

    def random_uniform(shape, minval=0, maxval=None, dtype=tf.float32, seed=None, name=None):
        shape = tuple(tf._ints(list(shape))) if len(shape) else ()
        if dtype is tf.int32:
            v = RNG[0].integers(int(minval), int(maxval), size=shape).astype(np.int32)
        else:
            hi = 1.0 if maxval is None else maxval
            u = RNG[0].random(size=shape, dtype=np.float32)
            v = u * np.float32(hi - minval) + np.float32(minval)      # TF: rnd * (maxval - minval) + minval
            assert v.dtype == np.float32
        DRAWS.append(np.array(v))
        return T(v)

    def map_fn(fn, elems, dtype=None, **kw):
        n = len(_a(elems[0]))
        rows = [fn(tuple(T(_a(e)[t]) for e in elems)) for t in range(n)]
        return tuple(T(np.stack([np.asarray(_a(r[k])) for r in rows])) for k in range(len(rows[0])))

    def tf_slice(x, begin, size, name=None):
        x, b, s = _a(x), tf._ints(list(_a(begin))), tf._ints(list(_a(size)))
        for d in range(x.ndim):
            if b[d] < 0 or b[d] + s[d] > x.shape[d]:
                raise ValueError("slice: begin %r size %r does not fit %r" % (b, s, x.shape))
        return T(x[tuple(slice(b[d], b[d] + s[d]) for d in range(x.ndim))])

    def resize_images(image, size, **kw):
        h, w = tf._ints(list(_a(size)))
        return T(O.tf_resize_bilinear(_a(image), h, w))

    def rotate(image, angles, interpolation="NEAREST", name=None):
        assert interpolation == "BILINEAR"
        img = _a(image)
        return T(O.tf_rotate_bilinear(img, O.rotate_transform(np.float32(_a(angles).reshape(())), img.shape[0])))

    ops = dict(
        random_uniform=random_uniform, map_fn=map_fn, slice=tf_slice,
        cond=lambda pred, a, b, **kw: a() if bool(_a(pred)) else b(),
        fill=lambda dims, value, name=None: T(np.full(tf._ints(list(dims)), _a(value))),
        less=lambda x, y, name=None: T(np.less(_a(x), _w(y))),
        cumsum=lambda x, axis=0, **kw: T(np.cumsum(_a(x), axis=axis, dtype=_a(x).dtype)),
        abs=lambda x, name=None: T(np.abs(_a(x))),
        reverse=lambda x, axis, name=None: T(np.flip(_a(x), axis=tuple(axis))),
        to_int32=lambda x, name=None: T(np.asarray(_a(x)).astype(np.int32)),         # truncates toward zero, like TF's cast
        to_float=lambda x, name=None: T(np.asarray(_a(x)).astype(np.float32)),
        transpose=lambda x, perm=None, name=None: T(np.transpose(_a(x), perm)),
        where=lambda c, x, y, name=None: T(np.where(_a(c), _a(x), _a(y))),
        acos=lambda x, name=None: T(np.arccos(_a(x))),
        sqrt=lambda x, name=None: T(np.sqrt(_a(x))),
        trace=lambda x, name=None: T(np.trace(_a(x), axis1=-2, axis2=-1)),
        clip_by_value=lambda x, lo, hi, name=None: T(np.clip(_a(x), np.asarray(lo, _a(x).dtype), np.asarray(hi, _a(x).dtype))),
        size=lambda x, name=None: int(np.size(_a(x))),
        subtract=lambda x, y, name=None: T(np.subtract(_a(x), _w(y))),
        multiply=lambda x, y, name=None: T(np.multiply(_a(x), _w(y))),
    )
    for k, v in ops.items():
        assert not hasattr(tf, k), k
        setattr(tf, k, v)
    tf.image = types.SimpleNamespace(resize_images=resize_images)
    tf.contrib.image = types.SimpleNamespace(rotate=rotate)
    return list(ops) + ["image"]


def main():
    from oracle import tf_shim
    import tube_oracle as O
    added = tf_shim.install(np.float32)
    names = extend_shim(tf_shim, O)
    sys.path.insert(0, REF)
    try:
        from src.util import tube_augmentation as TA
    finally:
        sys.path.remove(REF)

    S, T, H, W = 32, 6, 40, 52
    rng = np.random.default_rng(2026)
    images = rng.random((T, H, W, 3), dtype=np.float32)
    image_sizes = np.tile(np.array([[H, W]], np.int32), (T, 1))
    labels = np.stack([rng.uniform(4, W - 4, (T, 25)), rng.uniform(4, H - 4, (T, 25)), rng.integers(0, 2, (T, 25))], 1).astype(np.float32)
    centers = (np.array([[W // 2, H // 2]]) + rng.integers(-3, 4, (T, 2))).astype(np.int32)
    poses = rng.normal(0, 0.4, (T, 72)).astype(np.float32)
    gt3ds = rng.normal(0, 0.3, (T, 14, 3)).astype(np.float32)
    gt3ds -= gt3ds.mean(1, keepdims=True)
    ctor = dict(img_size=S, trans_max=6, delta_trans_max=2, scale_max=0.3, delta_scale_max=0.05)
    out = dict(images=images, image_sizes=image_sizes, labels=labels, centers=centers, poses=poses, gt3ds=gt3ds,
               ctor=np.array([ctor[k] for k in ("img_size", "trans_max", "delta_trans_max", "scale_max", "delta_scale_max")], np.float64),
               delta_rotate_max=np.float64(0.1))
    case = 0
    for want_flip in (False, True):
        for rotate_max in (0, 0.4):
            pre = TA.TubePreprocessor(rotate_max=rotate_max, delta_rotate_max=0.1 if rotate_max else 0, **ctor)
            seed = 0
            while True:                      # the flip is the reference's own first draw: take the first seed that gives the wanted one
                RNG[0] = np.random.default_rng(1000 * case + seed)
                del DRAWS[:]
                try:
                    r = pre(tf_shim.Tensor(images), tf_shim.Tensor(image_sizes), tf_shim.Tensor(labels), tf_shim.Tensor(centers),
                            tf_shim.Tensor(poses), tf_shim.Tensor(gt3ds), return_walk=True)
                except ValueError:
                    seed += 1
                    continue
                if bool(DRAWS[0] < 0.5) == want_flip:
                    break
                seed += 1
            p = "c%d_" % case
            out[p + "flip"] = np.bool_(want_flip)
            out[p + "rotate_max"] = np.float64(rotate_max)
            for i, d in enumerate(DRAWS):
                out[p + "draw%d" % i] = d
            out[p + "n_draws"] = np.int32(len(DRAWS))
            for k, v in r.items():
                v = np.asarray(tf_shim._a(v))
                assert v.dtype in (np.float32, np.int32), (k, v.dtype)
                out[p + k] = v
            print(case, "seed", seed, "flip", want_flip, "rotate_max", rotate_max, {k: out[p + k].shape for k in r})
            case += 1
    path = os.path.join(HERE, "reference_tube.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k in names:
        delattr(tf_shim, k)
    tf_shim.uninstall(added)


if __name__ == "__main__":
    main()
