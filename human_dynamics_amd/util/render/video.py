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

`video_bboxes` and `render_person_clips` are the reference's person-centred view (compute_video_bbox / visualize_mesh_og,
src/util/render/nmr_renderer.py:519-634, :422-488) for all tracks of a video: one hmmr_video_bbox call finds every person's
box and the cameras relative to it, and each view of a person is one hmmr_render_mesh call at the size of the box.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from ... import _lib as L
from .collage import compose_collage, skeleton_panels
from .handoff import orig_image_geometry
from . import person_view, raster
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


def _cams(records, layout, device):
    """rows [n, >= 3] read in place"""
    if isinstance(records, dict):
        c = records["cams"]
        c = torch.as_tensor(np.asarray(c, np.float32) if not torch.is_tensor(c) else c, device=device).float()
        return c.flatten(1) if c.dim() > 1 else c.reshape(-1, 3)          # (flatten: a track without frames has no -1 to infer)
    oc, sc, _ = {k: (off, size, shp) for k, shp, off, size in layout}["cams"]
    return records[:, oc:oc + sc]


def _kps(records, layout, device):
    """(rows [n, >= 2 K] read in place, K)"""
    if isinstance(records, dict):
        k = records["kps"]
        k = torch.as_tensor(np.asarray(k, np.float32) if not torch.is_tensor(k) else k, device=device).float()
        return k.flatten(1), int(k.shape[1])
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


def _records_in_place(tracks):
    """The tracks' packed records as ONE [N, ld] view when they lie end to end in one buffer, in order (what
    Tester.predict_tracks(records=True) returns): (rows, offsets), else None."""
    recs = [t[0] for t in tracks]
    if not all(torch.is_tensor(r) and r.dim() == 2 and r.dtype == torch.float32 and r.device.type == "cuda" for r in recs):
        return None
    layouts = [t[1] for t in tracks]
    width = recs[0].shape[1]
    ld = next((r.stride(0) for r in recs if r.shape[0] > 1), width)
    base = recs[0].untyped_storage().data_ptr()
    offsets = [0]
    first = recs[0].storage_offset()
    for r, lay in zip(recs, layouts):
        if (lay is not layouts[0] and lay != layouts[0]) or r.shape[1] != width or r.untyped_storage().data_ptr() != base:
            return None
        if r.shape[0] and (r.stride(1) != 1 or (r.shape[0] > 1 and r.stride(0) != ld)):
            return None
        if r.shape[0] and r.storage_offset() != first + offsets[-1] * ld:          # (an empty view may point anywhere)
            return None
        offsets.append(offsets[-1] + r.shape[0])
    n = offsets[-1]
    if n == 0:
        return None
    rows = torch.as_strided(recs[0], (n, width), (ld, 1), first)
    return rows, np.asarray(offsets, np.int32)


def video_bboxes(tracks, frame_hw, margin=10, device=None):
    """The video-level box of every tracked person and the cameras relative to it, in ONE hmmr_video_bbox call
    (compute_video_bbox of the reference, per track).

    tracks: the list render_scene takes -- per track (records_or_dict, layout, (start, end), image_og_params).  Packed records
    that lie end to end in one buffer (Tester.predict_tracks(records=True)) are read in place, cams and kps inside the records;
    otherwise (dicts, or separate buffers) the tracks' cams / kps rows are laid end to end first (torch.cat: plumbing).  The
    per-frame {scale, start_x, start_y} of image_og_params is the one upload (24 bytes a frame), the boxes and status words
    the one download (20 bytes a track).
    -> (bbox int32 [T,4] = {ymin, ymax, xmin, xmax} and status int32 [T] (_lib.BBOX_* bits) on the host, and between them
    cams_crop: per track a float32 [n_t, 3] DEVICE view of one buffer): (bbox, cams_crop, status)."""
    if not tracks:
        raise ValueError("no tracks")
    if device is None:
        r0 = tracks[0][0]
        r0 = r0["cams"] if isinstance(r0, dict) else r0
        device = r0.device if torch.is_tensor(r0) and r0.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    for t, (records, layout, (start, end), params) in enumerate(tracks):
        n_t = (records["cams"] if isinstance(records, dict) else records).shape[0]
        if len(params) != n_t or end - start != n_t:
            raise ValueError("track %d: %d rows, %d image_og_params, range (%d, %d)" % (t, n_t, len(params), start, end))
    proc_size = next((float(p[0]["im_shape"][0]) for _, _, _, p in tracks if len(p)), 224.0)
    proc = torch.as_tensor(np.concatenate([person_view.proc_rows(p) for _, _, _, p in tracks]), device=device)
    placed = _records_in_place(tracks)
    if placed is not None:
        rows, offsets = placed
        get = {k: (off, size, shp) for k, shp, off, size in tracks[0][1]}
        (oc, sc, _), (ok, sk, shp_k) = get["cams"], get["kps"]
        cams, kps, k = rows[:, oc:oc + sc], rows[:, ok:ok + sk], int(shp_k[0])
    else:
        cs, ks, k = [], [], None
        for records, layout, _, _ in tracks:
            kr, k = _kps(records, layout, device)
            cs.append(_cams(records, layout, device)[:, :3])
            ks.append(kr[:, :2 * k])
        offsets = np.zeros(len(tracks) + 1, np.int32)
        np.cumsum([c.shape[0] for c in cs], out=offsets[1:])
        cams, kps = torch.cat(cs).contiguous(), torch.cat(ks).contiguous()
    n = int(offsets[-1])
    if n == 0:                                         # nothing to read: every track is EMPTY by definition
        cams = kps = torch.zeros((0, max(3, 2 * k)), dtype=torch.float32, device=device)
    bbox, crop, status = person_view.video_bbox(cams, kps, k, proc, offsets, frame_hw, margin, proc_size=proc_size)
    host = torch.cat([bbox, status[:, None]], 1).cpu().numpy()                      # the one synchronisation point
    return host[:, :4].copy(), [crop[int(offsets[t]):int(offsets[t + 1])] for t in range(len(tracks))], host[:, 4].copy()


def check_track_ranges(tracks, n_frames):
    """ValueError naming the first track whose (start, end) does not lie inside the video's n_frames frames"""
    for t, (_, _, (start, end), _) in enumerate(tracks):
        if not 0 <= start <= end <= n_frames:
            raise ValueError("track %d: range (%d, %d) outside the %d frames" % (t, start, end, n_frames))


def clip_skip_reason(bbox, status, size):
    """None, or why no clip can be rendered for a track with this box, status word and clip_size"""
    h, w, S = size
    if status & person_view.BBOX_SKIP:
        return "status %s" % person_view.status_words(status)
    if h < 1 or w < 1:
        return "a window of %d x %d pixels" % (h, w)
    if not L.RENDER_MIN_SIZE <= S <= L.RENDER_MAX_SIZE:
        return "a side of %d pixels, outside [%d, %d]" % (S, L.RENDER_MIN_SIZE, L.RENDER_MAX_SIZE)
    return None


def person_clip_views(verts, cams_crop, faces, bbox, size, color, degs=(0, 90), frames=None):
    """{deg: uint8 [n, h', w', 3]} for n frames of one track: one hmmr_render_mesh call per angle at size S with the cameras
    of video_bboxes, trimmed to (h', w') (size = person_view.clip_size(bbox)).  frames: the track's n original frames uint8
    [n,H,W,3] on the device -- their window [ymin:ymax, xmin:xmax] is the background of the deg == 0 view -- or None: white."""
    h, w, S = size
    views = {}
    for deg in degs:
        kw = {}
        if frames is not None and deg == 0:
            kw = dict(bg_mode=L.RENDER_BG_FRAME, bg_image=frames[:, int(bbox[0]):int(bbox[1]), int(bbox[2]):int(bbox[3])])
        views[deg] = render_mesh(verts, cams_crop, faces, S, rot=rodrigues(deg, 'y'), color=color, out_hw=(h, w), **kw)["rgb"]
    return views


def render_person_clips(tracks, frames_uint8, faces, degs=(0, 90), margin=10, max_img_size=300, background=True, colors=None,
                        device=None):
    """One person-centred clip per tracked person: the reference's visualize_mesh_og with the box of compute_video_bbox, for
    every track and every angle of `degs`.

    tracks: as for render_scene; frames_uint8 [F,H,W,3] the original frames, row f - start of a track being the person in
    frame f.  Per track -> {'bbox': [ymin, ymax, xmin, xmax], 'status': the _lib.BBOX_* word, 'size': (h', w', S),
    'views': {deg: uint8 [n_t, h', w', 3] on the device}}: (h', w') is the box's window, down-scaled with resize_img's floor
    where its longer side exceeds max_img_size, S the longer side.  Each view is one hmmr_render_mesh call at size S with the
    track's cams_crop and the mesh turned by deg about y through its centroid, trimmed to (h', w').  The views are on white, as
    the reference's are -- except that with background=True the deg == 0 view is drawn over the frames' window
    [ymin:ymax, xmin:xmax] (resized by HMMR_RENDER_BG_FRAME's taps): that overlay is this project's addition, the reference
    renders its person-centred view on white only.
    A track whose status has EMPTY, NOT_FINITE or DEGENERATE, whose window has no pixel, or whose S lies outside
    [_lib.RENDER_MIN_SIZE, _lib.RENDER_MAX_SIZE] gets views = {} and a warning that names it; the other tracks are rendered.
    colors: per track as raster.scene_color takes them."""
    if device is None:
        r0 = tracks[0][0]
        r0 = r0["cams"] if isinstance(r0, dict) else r0
        device = r0.device if torch.is_tensor(r0) and r0.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces)
    fr = frames_uint8 if torch.is_tensor(frames_uint8) else torch.from_numpy(np.ascontiguousarray(frames_uint8))
    fr = fr.to(device)
    check_track_ranges(tracks, fr.shape[0])
    bbox, crops, status = video_bboxes(tracks, fr.shape[1:3], margin, device=device)
    out = []
    for t, (records, layout, (start, end), _) in enumerate(tracks):
        h, w, S = person_view.clip_size(bbox[t], max_img_size)
        res = {"bbox": bbox[t], "status": int(status[t]), "size": (h, w, S), "views": {}}
        out.append(res)
        why = clip_skip_reason(bbox[t], int(status[t]), res["size"])
        if why:
            warnings.warn("render_person_clips: track %d is not rendered (%s, box %s)" % (t, why, [int(x) for x in bbox[t]]))
            continue
        _, verts = _cams_verts(records, layout, device)
        res["views"] = person_clip_views(verts, crops[t], faces, bbox[t], res["size"], raster.scene_color(t, colors), degs,
                                         fr[start:end] if background else None)
    return out
