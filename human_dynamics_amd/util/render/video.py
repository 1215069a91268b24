"""The panels of the demo's `render_preds` (src/evaluation/run_video.py:110-202) for all n frames at once:

    render_og  visualize_img_orig's mesh over the original frame (down-scaled to max_img_size, make_square, remove_pads)
    rot_og     the same camera, the mesh rotated 90 deg about y through its centroid, on white (VisRenderer.rotated)
    rend_crop  visualize_img's mesh over the 224x224 crop
    skel_crop  visualize_img's 2D skeleton over the crop (view 'skel', one hmmr_draw_skeleton launch)
    collage    | rend_crop | render_og |  (view 'collage', one hmmr_compose_collage launch over the four panels)
               | skel_crop | rot_og    |

Each panel is one hmmr_render_mesh call (three launches per 64 frames) reading cams / verts in place inside the packed
per-frame records; the camera change to the original image is the device code of hmmr_render_handoff, so nothing
crosses PCIe until the caller downloads uint8 frames: with views=('collage',) the finished collage frames (and, for
render_preds' second folder, the 'orig' panel).  PNG and mp4 writing is evaluation/run_video.render_preds'; `draw_text`
(cv2.putText) is not provided.  The skeleton's draw list is the reference's, executed; the pixels of its discs, rings and
lines follow the integer rules of include/hmmr_hip.h, and their agreement with OpenCV's scan conversion at primitive
boundaries has not been measured.

`render_scene` is not the reference's: it draws ALL tracks of a video into each original frame in one hmmr_render_scene call
(the reference renders one track per video), layering the persons of a frame by camera scale; see include/hmmr_hip.h.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib as L
from .collage import compose_collage, skeleton_panels
from .handoff import orig_image_geometry
from . import raster
from .raster import COLORS, MeshFaces, render_mesh, rodrigues


def orig_output_size(frame_hw, max_img_size=720):
    """(h', w', S): the frame after visualize_img_orig's optional down-scale (resize_img's floor) and the square side."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    if max(h, w) > max_img_size:
        s = max_img_size / float(max(h, w))
        h, w = int(np.floor(h * s)), int(np.floor(w * s))
    return h, w, max(h, w)


def _cams_verts(records, layout, device):
    if isinstance(records, dict):                      # Tester.predict_all_images' dict (host or device)
        cams = torch.as_tensor(np.asarray(records["cams"], np.float32) if not torch.is_tensor(records["cams"])
                               else records["cams"], device=device).float()
        verts = torch.as_tensor(np.asarray(records["verts"], np.float32) if not torch.is_tensor(records["verts"])
                                else records["verts"], device=device).float()
        return cams.reshape(cams.shape[0], -1), verts
    get = {k: (off, size, shp) for k, shp, off, size in layout}
    oc, sc, _ = get["cams"]
    ov, sv, shp_v = get["verts"]
    return records[:, oc:oc + sc], records[:, ov:ov + sv].unflatten(1, tuple(shp_v))


def _kps(records, layout, device):
    """(rows [n, >= 2 K] read in place, K)"""
    if isinstance(records, dict):
        k = records["kps"]
        k = torch.as_tensor(np.asarray(k, np.float32) if not torch.is_tensor(k) else k, device=device).float()
        return k.reshape(k.shape[0], -1), int(k.shape[1])
    ok, sk, shp = {k: (off, size, shp) for k, shp, off, size in layout}["kps"]
    return records[:, ok:ok + sk], int(shp[0])


def render_views(records, layout, frames_uint8, image_og_params, faces, crops=None, views=('orig', 'rotated', 'crop'),
                 max_img_size=720, mesh_color='blue', device=None):
    """records [n, rec_len] packed per-frame records (Tester.predict_records, dist.record_layout) or the dict of
    predict_all_images; frames_uint8 [n,H,W,3] original frames; image_og_params: n dicts of process_image (start_pt,
    scale, im_shape); faces [F,3] (or a MeshFaces); crops [n,224,224,3] in [-1, 1] for the crop panel.
    -> {'orig': uint8 [n,h',w',3], 'rotated': uint8 [n,h',w',3], 'crop': uint8 [n,224,224,3]} on the device.
    Further view names: 'skel' uint8 [n,224,224,3], the predicted 2D skeleton over the crop, and 'collage' uint8
    [n, 448, 224 + max(w' 224 // h', 224), 3], render_preds' frame, which implies (and returns) the other four."""
    if 'collage' in views:
        views = tuple(views) + ('orig', 'rotated', 'crop', 'skel')
    if device is None:
        device = records.device if torch.is_tensor(records) else torch.device("cuda", torch.cuda.current_device())
    faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces)
    cams, verts = _cams_verts(records, layout, device)
    n = verts.shape[0]
    color = COLORS[mesh_color]
    out = {}
    if 'orig' in views or 'rotated' in views:
        h, w, S = orig_output_size(frames_uint8.shape[1:3], max_img_size)
        geom = np.stack([orig_image_geometry(image_og_params[i], frames_uint8.shape[1:3], max_img_size) for i in range(n)])
        if 'orig' in views:
            fr = frames_uint8 if torch.is_tensor(frames_uint8) else torch.from_numpy(np.ascontiguousarray(frames_uint8))
            out['orig'] = render_mesh(verts, cams, faces, S, geom=geom, color=color, bg_mode=L.RENDER_BG_FRAME,
                                      bg_image=fr.to(device), out_hw=(h, w))["rgb"]
        if 'rotated' in views:
            out['rotated'] = render_mesh(verts, cams, faces, S, geom=geom, rot=rodrigues(90, 'y'), color=color,
                                         out_hw=(h, w))["rgb"]
    if 'crop' in views:
        if crops is None:
            raise ValueError("the crop panel needs the 224x224 crops")
        cr = torch.as_tensor(crops, device=device).float()
        out['crop'] = render_mesh(verts, cams, faces, cr.shape[1], color=color, bg_mode=L.RENDER_BG_FLOAT, bg_image=cr,
                                  bg_add=1.0, bg_mul=127.5)["rgb"]
    if 'skel' in views:
        if crops is None:
            raise ValueError("the skeleton panel needs the 224x224 crops")
        cr = torch.as_tensor(crops, device=device).float()
        rows, nk = _kps(records, layout, device)             # ((kp + 1) * 0.5) * img_size and ((img + 1) * 0.5) * 255, fused
        out['skel'] = skeleton_panels(rows, cr, nk=nk, kp_add=1.0, kp_mul=0.5 * cr.shape[1], bg_add=1.0, bg_mul=127.5)
    if 'collage' in views:
        out['collage'] = compose_collage(out['crop'], out['skel'], out['orig'], out['rotated'])
    return out


def render_scene(tracks, frames_uint8, faces, max_img_size=720, colors=None, priority=None, device=None):
    """Every tracked person over the original frames, one raster per frame (hmmr_render_scene; the layering rule is this
    project's, the reference has no multi-person view).

    tracks: a list of (records_or_dict, layout, (start, end), image_og_params) per track: what predict_videos /
    predict_records (packed records + layout) or predict_all_images (a dict, layout None) return for the track, its frame
    range in frames_uint8 [F,H,W,3] and the end - start dicts of process_tracks / process_image.  Row f - start of a
    track is the person in frame f; cams / verts are read in place.  The geom rows come from orig_image_geometry, as in
    render_views.  A frame's persons are layered by `priority[t]` ([end - start] keys, larger in front) where given, else
    by the scale of the camera in the original image, larger in front; ties go to the lower track.
    colors: per track a raster.COLORS name or an rgb triple; the default cycles through raster.SCENE_COLORS ('blue',
    'pink', 'mint', 'orange', 'yellow', 'green', 'red', 'mint2', 'green2') by track index.
    -> uint8 [F, h', w', 3] on the device, (h', w') = orig_output_size(frame, max_img_size)[:2]."""
    if device is None:
        r0 = tracks[0][0]
        device = r0.device if torch.is_tensor(r0) else torch.device("cuda", torch.cuda.current_device())
    faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces)
    hw = tuple(frames_uint8.shape[1:3])
    h, w, S = orig_output_size(hw, max_img_size)
    fr = frames_uint8 if torch.is_tensor(frames_uint8) else torch.from_numpy(np.ascontiguousarray(frames_uint8))
    scene = []
    for t, (records, layout, (start, end), params) in enumerate(tracks):
        cams, verts = _cams_verts(records, layout, device)
        if len(params) != end - start:
            raise ValueError("track %d: %d image_og_params for the range (%d, %d)" % (t, len(params), start, end))
        geom = np.stack([orig_image_geometry(params[i], hw, max_img_size) for i in range(end - start)])
        scene.append({"verts": verts, "cams": cams, "range": (start, end), "geom": geom,
                      "priority": priority[t] if priority is not None else None})
    return raster.render_scene(scene, faces, S, fr.shape[0], colors=colors, bg_mode=L.RENDER_BG_FRAME, bg_image=fr.to(device),
                               out_hw=(h, w))["rgb"]
