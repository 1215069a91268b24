"""Mirror of src/evaluation/eval.py: scores one tube of predictions against its ground truth and accumulates the
per-dataset rows of the paper's table (doc/eval.md), with every metric evaluated on the device.

    compute_errors_batched  the reference's signature and dictionary, from arrays or device tensors
    score_records           the same dictionary straight from the packed per-frame records of Tester.predict_records
                            (dist.record_layout): kps, joints, poses and shapes are read in place through the strided entry
                            points of csrc/eval_metrics.hip, the four SMPL evaluations of the mesh errors run in chunks
                            and are compared by hmmr_eval_verts -- no mesh and no record leaves the device
    test_sequence[_const]   one tube, with the reference's pickle cache / its five past-present-future slices
    evaluate                the accumulation of main() (eval.py:382-493) over tubes that are already in memory

Reading `.tfrecord` files needs TensorFlow and is out of scope: `evaluate` takes, per dataset, an iterable of
`(tf_path, p_id, data)` with `data` the dictionary `read_from_example` returns (images, kps, gt3ds, poses, shape).
"""
from __future__ import annotations

import json
import os
import pickle
from time import time

import numpy as np
import torch

from .. import _lib as L
from . import eval_util as E
from .eval_util import extend_dict_entries, mean_of_dict_values, update_dict_entries
from .prediction import get_eval_path_name, get_predictions, get_result_path_name

DATASETS_3D = ["3dpw", "h36m"]
CONST_KEYS = ("past", "past_const", "present", "future", "future_const")
SMPL_CHUNK = 256                  # frames per SMPL evaluation of the mesh errors: two meshes of 83 KB per frame at a time

def _need_engine(engine):
    if engine is None:
        raise L.HmmrError("the mesh errors need the SMPL kernel: pass engine=<HmmrEngine> (Tester.engine)")
    return engine


def _theta_beta(engine, poses, shapes):
    dev = engine.device
    poses = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32))
    theta = poses.to(dev, torch.float32).reshape(poses.shape[0], 72)
    shapes = shapes if isinstance(shapes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(shapes, dtype=np.float32))
    return theta, shapes.to(dev, torch.float32)


def _smpl_chunks(engine, theta, beta, chunk):
    """(first frame, vertices, joints) of HmmrEngine.smpl over `chunk` frames at a time: the one loop behind compute_gpu_smpl
    and the mesh errors.  theta None is the T-pose."""
    n = beta.shape[0]
    zeros = torch.zeros((min(n, chunk), 72), dtype=torch.float32, device=engine.device) if theta is None else None
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        v, j, _, _ = engine.smpl(zeros[:m] if theta is None else theta[i:i + m], beta[i:i + m], want_rs=False)
        yield i, v, j


def compute_gpu_smpl(poses, shapes, get_joints=False, engine=None, chunk=SMPL_CHUNK):
    """SMPL vertices [N,V,3] (and the joints [N,K,3]) of axis-angle poses [N,72] and shapes [N,10] as device tensors
    (eval.py:68-90), from HmmrEngine.smpl in chunks of `chunk` frames so that the kernel's workspace stays bounded."""
    engine = _need_engine(engine)
    theta, beta = _theta_beta(engine, poses, shapes)
    n = theta.shape[0]
    verts = torch.empty((n, engine.num_verts, 3), dtype=torch.float32, device=engine.device)
    joints = torch.empty((n, engine.num_kps, 3), dtype=torch.float32, device=engine.device) if get_joints else None
    for i, v, j in _smpl_chunks(engine, theta, beta, chunk):
        verts[i:i + len(v)] = v
        if get_joints:
            joints[i:i + len(j)] = j
    return (verts, joints) if get_joints else verts


def _mesh_errors(poses_gt, shapes_gt, poses_pred, shapes_pred, engine, chunk=SMPL_CHUNK):
    """Per-frame mean vertex distance between the ground-truth and the predicted SMPL mesh, posed and in the T-pose
    (eval.py:157-174), as two device tensors [N].  A chunk of frames at a time: four SMPL evaluations and two
    hmmr_eval_verts launches, so 2 x chunk meshes exist at once instead of 4 x N."""
    engine = _need_engine(engine)
    tg, bg = _theta_beta(engine, poses_gt, shapes_gt)
    tp, bp = _theta_beta(engine, poses_pred, shapes_pred)
    n = tg.shape[0]
    assert tp.shape[0] == n and bg.shape[0] == n and bp.shape[0] == n, (tg.shape, tp.shape, bg.shape, bp.shape)
    posed = torch.empty(n, dtype=torch.float32, device=engine.device)
    tpose = torch.empty(n, dtype=torch.float32, device=engine.device)
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    for out, pose_g, pose_p in ((tpose, None, None), (posed, tg, tp)):
        for (i, vg, _), (_, vp, _) in zip(_smpl_chunks(engine, pose_g, bg, chunk), _smpl_chunks(engine, pose_p, bp, chunk)):
            m, nv = vg.shape[0], vg.shape[1]
            L.check(L.load().hmmr_eval_verts(vg.data_ptr(), nv * 3, vp.data_ptr(), nv * 3, m, nv, out[i:i + m].data_ptr(), stream),
                    "hmmr_eval_verts")
    return posed, tpose


def _joint_metrics_ld(gt, pred, device, want_err):
    """hmmr_eval_joints_ld on [n,k,3] inputs read in place: (mpjpe, pa_mpjpe, accel, accel_err) device tensors or None."""
    pred, ld_pred = E._rows(pred, device, (3,))
    n, k = pred.shape[0], pred.shape[1]
    ld_gt = 3 * k
    if gt is not None:
        gt, ld_gt = E._rows(gt, device, (3,))
        assert gt.shape[:2] == pred.shape[:2], (tuple(gt.shape), tuple(pred.shape))
    mp = torch.empty(n, device=device) if want_err else None
    pa = torch.empty(n, device=device) if want_err else None
    ac = torch.empty(max(n - 2, 0), device=device)
    ae = torch.empty(max(n - 2, 0), device=device) if gt is not None else None
    if n == 0:                                                        # as kp_metrics_device: an empty tube has empty results
        return mp, pa, ac, ae
    L.check(L.load().hmmr_eval_joints_ld(L.ptr(gt), ld_gt, pred.data_ptr(), ld_pred, n, k, E.LEFT_HIP, E.RIGHT_HIP, L.ptr(mp),
                                         L.ptr(pa), ac.data_ptr(), L.ptr(ae), torch.cuda.current_stream(device).cuda_stream),
            "hmmr_eval_joints_ld")
    return mp, pa, ac, ae


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def compute_errors_batched(kps_gt,
                           kps_pred,
                           joints_gt=None,
                           joints_pred=None,
                           poses_gt=None,
                           poses_pred=None,
                           shape_gt=None,
                           shapes_pred=None,
                           img_size=224,
                           has_3d=False,
                           min_visible=6,
                           compute_mesh=False,
                           engine=None,
                           device=None,
                           keep_device=False):
    """Computes the errors of one tube (eval.py:114-193): the dictionary with 'accel', 'kp', 'kp_pa', 'kp_pck' and, with
    has_3d, 'accel_error', 'mesh_posed', 'mesh_tpose', 'pose', 'joints', 'joints_pa', 'shape' ('pose' and 'shape' are the
    reference's literal -1, the mesh errors too without compute_mesh).  Inputs are arrays or device tensors; device views are
    read in place.  kps_pred is in [-1, 1] and is brought to image space in the kernel.  With compute_mesh the four SMPL
    evaluations come from `engine` and only the per-frame errors reach the host.  keep_device adds '_device': the per-frame
    device tensors the entries were read from, before the visibility selection."""
    if device is None:
        device = engine.device if engine is not None else "cuda:0"
    e_kp, e_kp_pa, e_pck, _ = E.kp_metrics_device(kps_gt, kps_pred, alpha=0.05 * img_size, min_visible=min_visible,
                                                   img_size=img_size, device=device)
    gt3 = None
    if has_3d:
        gt3 = joints_gt if isinstance(joints_gt, torch.Tensor) else np.asarray(joints_gt)
        gt3 = gt3.reshape(len(gt3), -1, 3)
    mp, pa, accel, accel_err = _joint_metrics_ld(gt3, joints_pred, device, want_err=has_3d)
    dev_out = {"kp": e_kp, "kp_pa": e_kp_pa, "kp_pck": e_pck, "accel": accel}
    errors_dict = {
        'accel': _f64(accel),
        'kp': E._float_list(e_kp),
        'kp_pa': E._float_list(e_kp_pa),
        'kp_pck': E._float_list(e_pck),
    }
    if has_3d:
        vis = np.sum(_host(kps_gt)[:, :14, 2], axis=1) > min_visible
        invis = np.logical_not(vis)
        new_vis = np.logical_not(np.logical_or(invis, np.logical_or(np.roll(invis, -1), np.roll(invis, -2)))[:-2])
        errors_pose, errors_shape = -1, -1
        if compute_mesh:
            n = len(vis)
            shape_gt_t = shape_gt if isinstance(shape_gt, torch.Tensor) else torch.from_numpy(np.asarray(shape_gt, np.float32))
            shapes_gt = shape_gt_t.reshape(1, 10).expand(n, 10).contiguous()                         # np.tile(shape_gt, (N, 1))
            aa_pred = E.rotmat_to_aa_device(poses_pred, device)                        # rot_mat_to_axis_angle per frame
            posed, tpose = _mesh_errors(poses_gt, shapes_gt, aa_pred, shapes_pred, engine)
            dev_out.update(mesh_posed=posed, mesh_tpose=tpose)
            errors_mesh_posed, errors_mesh_tpose = _f64(posed)[vis], _f64(tpose)[vis]
        else:
            errors_mesh_posed, errors_mesh_tpose = -1, -1
        dev_out.update(joints=mp, joints_pa=pa, accel_error=accel_err)
        mp_h, pa_h = _f64(mp), _f64(pa)
        errors_dict.update({
            'accel_error': _f64(accel_err)[new_vis],
            'mesh_posed': errors_mesh_posed,
            'mesh_tpose': errors_mesh_tpose,
            'pose': errors_pose,
            'joints': list(mp_h[vis]),
            'joints_pa': list(pa_h[vis]),
            'shape': errors_shape,
        })
    if keep_device:
        errors_dict['_device'] = dev_out
    return errors_dict


def score_records(records, layout, data, img_size=224, has_3d=False, min_visible=6, compute_mesh=False, engine=None,
                  keep_device=False):
    """`compute_errors_batched` straight from the packed per-frame records [n, rec_len] of Tester.predict_records
    (`layout` from Tester.record_layout / dist.record_layout) and the tube's ground truth `data` (kps, gt3ds, poses, shape):
    the kps / joints[:, :14] / poses / shapes fields are read where they lie, through the row strides of hmmr_eval_kps,
    hmmr_eval_joints_ld, hmmr_rotmat_to_axis_angle and the SMPL kernel.  Equal bit for bit to compute_errors_batched on the
    dictionary unpacked (and downloaded) from the same records."""
    from ..dist import unpack_outputs
    assert records.is_cuda and records.dtype == torch.float32 and records.dim() == 2 and records.stride(1) == 1
    fields = {k: (shp, off, size) for k, shp, off, size in layout}
    want = ("kps", "joints", "poses", "shapes")
    views = unpack_outputs(records, [(k,) + fields[k] for k in want])
    return compute_errors_batched(
        kps_gt=data['kps'],
        kps_pred=views['kps'],
        joints_gt=data['gt3ds'] if has_3d else None,
        joints_pred=views['joints'][:, :14],
        poses_gt=data.get('poses'),
        poses_pred=views['poses'],
        shape_gt=data.get('shape'),
        shapes_pred=views['shapes'],
        img_size=img_size,
        has_3d=has_3d,
        min_visible=min_visible,
        compute_mesh=compute_mesh,
        engine=engine,
        device=records.device,
        keep_device=keep_device,
    )


def test_sequence(data, preds, eval_path, pred_mode='pred', has_3d=False,
                  min_visible=6, compute_mesh=False, engine=None):
    """Tests one tube (eval.py:196-243): the error dictionary of `compute_errors_batched`, read from the pickle at
    `eval_path` when it exists and written there otherwise.  pred_mode 'hal' scores the centre prediction of the '_hal' keys."""
    img_size = np.shape(data['images'])[1]

    if pred_mode == 'hal':
        # The keys have a '_hal' suffix in them; only the centre prediction is wanted.
        preds = {k.replace('_hal', ''): v[:, 1] for k, v in preds.items() if '_hal' in k}

    if os.path.exists(eval_path):
        print('Eval already exists! {}'.format(eval_path))
        with open(eval_path, 'rb') as f:
            return pickle.load(f)
    t0 = time()
    errors = compute_errors_batched(
        kps_gt=data['kps'],
        kps_pred=preds['kps'],
        joints_gt=data['gt3ds'],
        joints_pred=preds['joints'][:, :14],
        poses_gt=data['poses'],
        poses_pred=preds['poses'],
        shape_gt=data['shape'],
        shapes_pred=preds['shapes'],
        img_size=img_size,
        has_3d=has_3d,
        min_visible=min_visible,
        compute_mesh=compute_mesh,
        engine=engine,
    )
    with open(eval_path, 'wb') as f:
        print('Saving eval to', eval_path)
        pickle.dump(errors, f)
    print('Eval time:', time() - t0)
    return errors


def test_sequence_const(data, preds, eval_path, has_3d=False, min_visible=6, delta_t=5, engine=None):
    """The constant baseline against the hallucinated past / future (eval.py:246-327): 'present' scores container 0 of the
    '_hal' predictions on every frame; 'past' / 'future' score containers 0 / 2 shifted by delta_t frames, and
    'past_const' / 'future_const' the centre container 1 with the same shift.  (The reference reads delta_t from its
    module-level config.)"""
    img_size = np.shape(data['images'])[1]
    kps_pred, joints_pred, poses_pred = preds['kps_hal'], preds['joints_hal'], preds['poses_hal']
    gt3ds = data['gt3ds']
    gt3ds = gt3ds.reshape(len(gt3ds), -1, 3) if hasattr(gt3ds, "reshape") else np.asarray(gt3ds).reshape(len(gt3ds), -1, 3)
    head, tail = slice(None, -delta_t), slice(delta_t, None)
    # name -> (ground-truth frames, predicted frames, container)
    plan = {
        'present': (slice(None), slice(None), 0),
        'past': (head, tail, 0),
        'past_const': (head, tail, 1),
        'future': (tail, head, 2),
        'future_const': (tail, head, 1),
    }
    errors_dict = {}
    for name, (g, p, c) in plan.items():
        errors_dict[name] = compute_errors_batched(
            kps_gt=data['kps'][g],
            kps_pred=kps_pred[p, c],
            joints_gt=gt3ds[g, :14],
            joints_pred=joints_pred[p, c, :14],
            poses_gt=data['poses'][g],
            poses_pred=poses_pred[p, c],
            img_size=img_size,
            has_3d=has_3d,
            min_visible=min_visible,
            engine=engine,
        )
    errors_dict = {k: errors_dict[k] for k in CONST_KEYS}
    with open(eval_path, 'wb') as f:
        print('Saving eval to', eval_path)
        pickle.dump(errors_dict, f)
    return errors_dict


def print_summary(errors_dict):
    """One row per dataset (eval.py:330-338)."""
    keys = ['accel', 'kp', 'kp_pa', 'kp_pck', 'joints', 'joints_pa', 'mesh_posed', 'mesh_tpose']
    print(('{:>15}' + '{:>11}' * len(keys)).format('Data', *keys))
    for dataset, errors in sorted(errors_dict.items()):
        print(('{:>15}' + '{:>11.5f}' * len(keys)).format(dataset, *[errors.get(key, -1) for key in keys]))


def save_results(config, all_dataset_results, json_path=''):
    """Writes the result rows as JSON when a path is given and prints them, per prediction type in 'const' mode
    (eval.py:341-350)."""
    if json_path:
        with open(json_path, 'w') as f:
            json.dump(all_dataset_results, f)
    if config.pred_mode == 'const':
        for pred_type, predictions in sorted(all_dataset_results.items()):
            print('Predicting', pred_type)
            print_summary(predictions)
    else:
        print_summary(all_dataset_results)


def evaluate(model, config, datasets, json_path=None):
    """The accumulation of the reference's main() (eval.py:382-493) -> `all_dataset_results`: {dataset: {metric: mean}} or,
    with config.pred_mode == 'const', {'past' | 'past_const' | 'present' | 'future' | 'future_const': {dataset: {...}}}.

    model: a Tester (its predict_all_images fills the prediction cache; its engine evaluates SMPL for the mesh errors).
    config: load_path, pred_mode, pred_dir, min_visible, split and, for 'const', delta_t.
    datasets: {name: iterable of (tf_path, p_id, data)} -- tubes already in memory, in the reference's order (its sorted
    tfrecord paths, the examples of each in file order); consecutive tubes with the same tf_path form one path result.
    Reading .tfrecord files needs TensorFlow and is out of scope.  Every tube goes through the reference's two caches:
    predictions under pred_dir (prediction.get_predictions) and the per-tube pickle of test_sequence.  json_path: where
    save_results writes the rows (None: get_result_path_name's; '': nowhere)."""
    const = config.pred_mode == 'const'
    engine = getattr(model, "engine", None)
    pred_dir = getattr(config, "pred_dir", "predictions_cache")
    nest = (lambda: {k: {} for k in CONST_KEYS}) if const else dict
    all_dataset_results = nest()
    for dataset, tubes in datasets.items():
        print('Evaluating dataset:', dataset)
        dataset_result = nest()
        path_result, path_name = None, None

        def close_path():
            if path_result is None:
                return
            if const:
                for k in path_result.keys():
                    update_dict_entries(dataset_result[k], path_result[k])
            else:
                update_dict_entries(dataset_result, path_result)

        for tf_path, p_id, data in tubes:
            if tf_path != path_name:
                close_path()
                path_result, path_name = nest(), tf_path
                print('\n', '*' * 10)
                print('Running on', os.path.basename(tf_path))
            preds = get_predictions(model=model, images=data['images'], load_path=config.load_path, tf_path=tf_path,
                                    p_id=p_id, pred_dir=pred_dir)
            eval_path = get_eval_path_name(load_path=config.load_path, pred_mode=config.pred_mode, tf_path=tf_path,
                                           p_id=p_id, pred_dir=pred_dir, min_visible=config.min_visible)
            if const:
                errors_dict = test_sequence_const(data=data, preds=preds, eval_path=eval_path,
                                                  has_3d=(dataset in DATASETS_3D), min_visible=config.min_visible,
                                                  delta_t=config.delta_t, engine=engine)
                for k in errors_dict.keys():
                    extend_dict_entries(path_result[k], errors_dict[k])
            else:
                compute_mesh = config.split == 'test' and dataset == '3dpw'
                errors = test_sequence(data=data, preds=preds, eval_path=eval_path, pred_mode=config.pred_mode,
                                       has_3d=(dataset in DATASETS_3D), min_visible=config.min_visible,
                                       compute_mesh=compute_mesh, engine=engine)
                extend_dict_entries(path_result, errors)
        close_path()

        if const:
            for pred_type, result in dataset_result.items():
                mean_of_dict_values(result)
                all_dataset_results[pred_type][dataset] = result
        else:
            mean_of_dict_values(dataset_result)
            all_dataset_results[dataset] = dataset_result

    if json_path is None:
        json_path = get_result_path_name(split=config.split, load_path=config.load_path, pred_mode=config.pred_mode,
                                         datasets=list(datasets), pred_dir=pred_dir)
    save_results(config, all_dataset_results, json_path)
    return all_dataset_results
