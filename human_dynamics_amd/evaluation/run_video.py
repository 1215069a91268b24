"""Device mirror of the crop in src/evaluation/run_video.py (`process_image`, :56-107).

    images, infos = process_images(frames_uint8[n,H,W,3], bbox_params[n,3])

returns the [n,224,224,3] float32 crops in [-1,1] as a DEVICE tensor (ready for
Tester.predict_all_images / ShardedPredictor) plus, per frame, the dict fields of the reference
(`im_shape`, `center`, `scale`, `start_pt`).  Decoding (imread) stays with the caller.

    per_track = process_tracks(frames_uint8[F,H,W,3], tracks_kps, vis_thresh=0.1)

is the front of demo_video.predict_on_tracks (:136-153) for any number of person tracks of one video: keypoints -> smoothed
boxes (util/smooth_bbox.py) -> crop integers -> crops, all on the device, with one download (ranges, status, info) at the end.

    render_preds(output_path, config, preds, images, images_orig, trim_length)

is `render_preds` (:110-202): the 2x2 collage frames and the full-size mesh-on-original frames of one track, rendered in
chunks on the device (util/render/video.render_views), written as PNGs with PIL and, where an ffmpeg is installed, turned
into the two mp4s by the reference's command line.  The skeleton's draw list is the reference's; the pixels of its
primitives follow the integer rules of include/hmmr_hip.h, whose agreement with OpenCV at primitive boundaries has not been
measured; no text is drawn.

    render_tracks(output_path, tracks, frames, faces=...)

is not the reference's (it renders one track per video): all tracks of a video over each original frame, one PNG per frame
and one mp4 (util/render/video.render_scene, include/hmmr_hip.h: hmmr_render_scene).

    render_person_clips(output_path, tracks, frames, faces=...)

is the reference's person-centred view (compute_video_bbox + visualize_mesh_og, src/util/render/nmr_renderer.py) as a driver,
which the reference does not have: one folder of PNGs and one mp4 per tracked person, cropped to the box that holds the
person over the whole video, the mesh seen from several angles side by side (util/render/video.render_person_clips,
include/hmmr_hip.h: hmmr_video_bbox).
"""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import torch

from .. import _lib as L
from ..util import smooth_bbox
from .tracks import pack_tracks

IMG_SIZE = 224


def crop_geometry(h, w, bbox_param):
    """The integers of process_image / resize_img for one frame, in the reference's float64
    arithmetic: scaled size, centre after scaling (x uses the HEIGHT factor and y the WIDTH factor,
    as `center * scale_factors` does at run_video.py:74), crop origin."""
    center = np.asarray(bbox_param[:2], np.float64)
    scale = float(bbox_param[2])
    new_size = (np.floor(np.array([h, w]) * scale)).astype(int)                 # common.py:8
    factors = [new_size[0] / float(h), new_size[1] / float(w)]
    center_scaled = np.round(center * factors).astype(int) + IMG_SIZE           # in the padded image
    start_pt = center_scaled - IMG_SIZE // 2
    hp, wp = new_size[0] + 2 * IMG_SIZE, new_size[1] + 2 * IMG_SIZE
    end_pt = np.array([min(center_scaled[0] + IMG_SIZE // 2, wp), min(center_scaled[1] + IMG_SIZE // 2, hp)])
    if new_size.min() < 1 or (end_pt - start_pt != IMG_SIZE).any() or (start_pt < 0).any():
        raise ValueError("bbox %s does not yield a full 224x224 crop of a %dx%d frame" % (bbox_param, h, w))
    return {"hs": int(new_size[0]), "ws": int(new_size[1]), "u0": int(start_pt[0] - IMG_SIZE),
            "v0": int(start_pt[1] - IMG_SIZE), "center": center_scaled - start_pt, "scale": scale,
            "start_pt": start_pt, "im_shape": [IMG_SIZE, IMG_SIZE]}


def process_images(frames, bbox_params, device="cuda:0"):
    lib = L.load()
    if isinstance(frames, torch.Tensor):
        fr = frames.to(device).contiguous()
    else:
        fr = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
    assert fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == 3, "frames: [n,H,W,3] uint8 (RGB)"
    n, h, w = fr.shape[:3]
    infos = [crop_geometry(h, w, bp) for bp in np.asarray(bbox_params, np.float64)]
    geom = torch.tensor([[g["hs"], g["ws"], g["u0"], g["v0"]] for g in infos], dtype=torch.int32).to(device)
    out = torch.empty((n, IMG_SIZE, IMG_SIZE, 3), dtype=torch.float32, device=device)
    L.check(lib.hmmr_crop_frames(fr.data_ptr(), geom.data_ptr(), n, h, w, out.data_ptr(),
                                 torch.cuda.current_stream(device).cuda_stream), "hmmr_crop_frames")
    return out, [{k: g[k] for k in ("im_shape", "center", "scale", "start_pt")} for g in infos]


def process_tracks(frames, tracks_kps, vis_thresh=0.1, kernel_size=11, sigma=3, device="cuda:0"):
    """frames: [F,H,W,3] uint8 (RGB), a device tensor or a host array that is uploaded once.  tracks_kps: [track][frame] ->
    (K,3) keypoints or None, frame i of every track being frames[i] (evaluation/tracks.get_labels_poseflow).

    Returns, per track, (crops, (start, end), infos): the [end-start,224,224,3] float32 device crops of frames[start:end] with
    the track's smoothed boxes -- bit for bit process_images(frames[start:end], smoothed[start:end]) -- and the images_orig
    dicts of those frames.  Nothing comes to the host between the keypoint upload and the one download at the end; a box that
    gives no full crop (or a track without a box) raises ValueError there, naming the track and its first bad frame.

    The extent of a track is not known on the host before that download, so every row of a track is cropped (rows outside
    [start, end) with the identity geometry) and `crops` is a view of rows [start, end) of a [len(track),224,224,3] buffer: a
    track with long leading or trailing gaps pays the crop work and keeps about 602 KB per unused frame alive for as long as
    the view lives.  `crops.clone()` releases it."""
    lib = L.load()
    if isinstance(frames, torch.Tensor):
        fr = frames.to(device).contiguous()
    else:
        fr = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
    assert fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == 3, "frames: [F,H,W,3] uint8 (RGB)"
    n_frames, h, w = fr.shape[:3]
    tracks_kps = [list(trk) for trk in tracks_kps]
    if not tracks_kps:
        return []
    for t, trk in enumerate(tracks_kps):
        if not 1 <= len(trk) <= n_frames:
            raise ValueError("track %d has %d entries for %d frames" % (t, len(trk), n_frames))
    kps, present, offsets = pack_tracks(tracks_kps)
    n, n_tracks = int(offsets[-1]), len(tracks_kps)
    dev, stream = fr.device, torch.cuda.current_stream(fr.device).cuda_stream
    smooth, rng, _ = smooth_bbox.track_boxes(torch.from_numpy(kps).to(dev), torch.from_numpy(present).to(dev), offsets, vis_thresh,
                                             kernel_size, sigma)
    # what the host needs at the end, in one buffer: info [N][5] float64 | range [T][2] int32 | status [N] int32
    blob = torch.empty(n * 40 + n_tracks * 8 + n * 4, dtype=torch.uint8, device=dev)
    info, rng_out, status = blob[:n * 40].view(torch.float64), blob[n * 40:n * 40 + n_tracks * 8].view(torch.int32), blob[n * 40 + n_tracks * 8:].view(torch.int32)
    geom = torch.empty((n, 4), dtype=torch.int32, device=dev)
    off_p = offsets.ctypes.data_as(L.C.POINTER(L.C.c_int32))
    L.check(lib.hmmr_track_crop_geom(smooth.data_ptr(), off_p, rng.data_ptr(), n_tracks, h, w, geom.data_ptr(), info.data_ptr(),
                                     status.data_ptr(), stream), "hmmr_track_crop_geom")
    rng_out.copy_(rng.reshape(-1))
    # every row of a track is cropped (rows outside [start, end) with the identity geometry): the extent is not known here
    crops = []
    for t in range(n_tracks):
        o, nt = int(offsets[t]), int(offsets[t + 1] - offsets[t])
        out = torch.empty((nt, IMG_SIZE, IMG_SIZE, 3), dtype=torch.float32, device=dev)
        L.check(lib.hmmr_crop_frames(fr.data_ptr(), geom[o:].data_ptr(), nt, h, w, out.data_ptr(), stream), "hmmr_crop_frames")
        crops.append(out)
    host = blob.cpu().numpy()                                                   # the one synchronisation point
    info_h = host[:n * 40].view(np.float64).reshape(n, 5)
    rng_h = host[n * 40:n * 40 + n_tracks * 8].view(np.int32).reshape(n_tracks, 2)
    status_h = host[n * 40 + n_tracks * 8:].view(np.int32)
    results = []
    for t in range(n_tracks):
        o, (start, end) = int(offsets[t]), (int(rng_h[t, 0]), int(rng_h[t, 1]))
        if start < 0:
            raise ValueError("track %d: no frame has a bounding box" % t)
        bad = np.flatnonzero(status_h[o:o + end])
        if len(bad):
            raise ValueError("track %d: the smoothed box of frame %d does not yield a full 224x224 crop of a %dx%d frame (status %d; "
                             "%d such frames)" % (t, bad[0], h, w, status_h[o + bad[0]], len(bad)))
        infos = [{"im_shape": [IMG_SIZE, IMG_SIZE], "center": row[2:4].astype(int), "scale": float(row[4]), "start_pt": row[:2].astype(int)}
                 for row in info_h[o + start:o + end]]
        results.append((crops[t][start:end], (start, end), infos))
    return results


def _ffmpeg_command(output_path, img_dir, fps=25):
    """make_video's command line (:205-225)"""
    return ['ffmpeg', '-y', '-threads', '16', '-framerate', str(fps), '-i', '{}/frame%06d.png'.format(img_dir),
            '-profile:v', 'baseline', '-level', '3.0', '-c:v', 'libx264', '-pix_fmt', 'yuv420p', '-an',
            '-vf', 'scale=trunc(iw/2)*2:trunc(ih/2)*2', output_path]


def make_video(output_path, img_dir, fps=25):
    """Runs ffmpeg over img_dir/frame%06d.png if there is one: True (written), False (ffmpeg failed) or None (no ffmpeg)."""
    if shutil.which('ffmpeg') is None:
        return None
    cmd = _ffmpeg_command(output_path, img_dir, fps)
    print(' '.join(cmd))
    try:
        return subprocess.call(cmd) == 0
    except OSError:
        return False


def _read_frames(images_orig, lo, hi):
    from PIL import Image
    return np.stack([np.asarray(Image.open(images_orig[j]['im_path']).convert("RGB")) for j in range(lo, hi)])


def render_preds(output_path, config, preds, images, images_orig, trim_length, img_size=224, frames=None, faces=None,
                 face_path='src/tf_smpl/smpl_faces.npy', chunk=64, device=None):
    """Renders frames [trim_length, len - trim_length) of one track as the reference does:

        output_path/frame%06d.png            the mesh over the original frame (down-scaled to at most 720 pixels)
        output_path + '_crop'/frame%06d.png  | mesh on the crop   | mesh on the original frame |
                                             | skeleton on crop   | mesh rotated 90 degrees    |

    preds: predict_all_images' dict (cams, kps, verts; host arrays or device tensors); images: the img_size crops in [-1, 1];
    images_orig: process_image's dicts (im_path, start_pt, scale, im_shape).  frames: the original frames uint8 [n,H,W,3]
    (host or device) instead of reading im_path with PIL; faces: [F,3] instead of reading face_path.
    Returns None if output_path + '.mp4' exists already ("Video already exists!"), else a dict: the two folders, the number
    of frames written, and `videos`: the mp4 paths, or None with `note` saying that no ffmpeg was found and the PNG frames
    were left in place."""
    from PIL import Image
    from ..util.render import video
    from ..util.render.nmr_renderer import load_faces
    from ..util.render.raster import MeshFaces
    max_img_size = 720
    output_crop = output_path + '_crop'
    vid_path, vid_path_crop = output_path + '.mp4', output_crop + '.mp4'
    if os.path.exists(vid_path):
        print('Video already exists!')
        return None
    for d in (output_path, output_crop):
        if not os.path.exists(d):
            os.mkdir(d)
    if device is None:
        v = preds['verts']
        device = v.device if torch.is_tensor(v) and v.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    mesh_faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces if faces is not None else load_faces(face_path))
    lo, hi = trim_length, len(preds['kps']) - trim_length
    written = 0
    for a in range(lo, hi, chunk):
        b = min(a + chunk, hi)
        part = {k: preds[k][a:b] for k in ('cams', 'kps', 'verts')}
        fr = frames[a:b] if frames is not None else _read_frames(images_orig, a, b)
        crops = images[a:b] if torch.is_tensor(images) else np.stack([np.asarray(images[j], np.float32) for j in range(a, b)])
        if tuple(crops.shape[1:3]) != (img_size, img_size):
            raise ValueError("crops of %s for img_size = %d" % (tuple(crops.shape[1:3]), img_size))
        out = video.render_views(part, None, fr, images_orig[a:b], mesh_faces, crops=crops, views=('collage',),
                                 max_img_size=max_img_size, mesh_color=config.mesh_color, device=device)
        full, collage = out['orig'].cpu().numpy(), out['collage'].cpu().numpy()
        for j in range(a, b):
            name = 'frame{:06d}.png'.format(j - trim_length)
            Image.fromarray(full[j - a]).save(os.path.join(output_path, name))
            Image.fromarray(collage[j - a]).save(os.path.join(output_crop, name))
            written += 1
    print('Converting them to video..')
    made = [make_video(vid_path, output_path), make_video(vid_path_crop, output_crop)]
    result = {"frames": output_path, "frames_crop": output_crop, "n_frames": written, "videos": None, "note": None}
    if made[0] is None:
        result["note"] = "no ffmpeg on PATH: the PNG frames are left in %s and %s" % (output_path, output_crop)
    elif all(made):
        result["videos"] = (vid_path, vid_path_crop)
    else:
        result["note"] = "ffmpeg failed: the PNG frames are left in %s and %s" % (output_path, output_crop)
    return result


def _clip_tracks(tracks, a, b, colors, priority):
    """The tracks present in frames [a, b), their rows and ranges cut to it: (tracks, colors, priority) for video.render_scene
    on frames[a:b].  Each keeps the colour of its index in the whole video."""
    from ..util.render.raster import scene_color
    part, cols, prio = [], [], []
    for t, (records, layout, (start, end), params) in enumerate(tracks):
        s, e = max(start, a), min(end, b)
        if s >= e:
            continue
        rows = slice(s - start, e - start)
        rec = {k: records[k][rows] for k in ('cams', 'verts')} if isinstance(records, dict) else records[rows]
        part.append((rec, layout, (s - a, e - a), params[rows]))
        cols.append(scene_color(t, colors))
        prio.append(priority[t][rows] if priority is not None and priority[t] is not None else None)
    return part, cols, prio


def render_tracks(output_path, tracks, frames, faces=None, face_path='src/tf_smpl/smpl_faces.npy', trim_length=0, chunk=64,
                  max_img_size=720, colors=None, priority=None, device=None):
    """Renders frames [trim_length, F - trim_length) of a video with ALL its tracks in each frame:

        output_path/frame%06d.png   every person present in the frame over the original frame (at most 720 pixels)

    tracks: per track (records_or_dict, layout, (start, end), image_og_params), as util/render/video.render_scene takes
    them; frames: uint8 [F,H,W,3], host or device.  The frames are rendered `chunk` at a time, each track cut to the
    chunk, and come to the host as finished uint8 frames.  colors / priority: as video.render_scene, per track of the
    whole video.  A chunk in which nobody is tracked shows the resized frames.
    Returns None if output_path + '.mp4' exists already ("Video already exists!"), else a dict: the folder, the number of
    frames written, and `video`: the mp4 path, or None with `note` saying that no ffmpeg was found (or that it failed)
    and the PNG frames were left in place."""
    from PIL import Image
    from ..util.render import video
    from ..util.render.nmr_renderer import load_faces
    from ..util.render.raster import MeshFaces
    vid_path = output_path + '.mp4'
    if os.path.exists(vid_path):
        print('Video already exists!')
        return None
    if not os.path.exists(output_path):
        os.mkdir(output_path)
    mesh_faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces if faces is not None else load_faces(face_path))
    if device is None:
        r0 = tracks[0][0]
        device = r0.device if torch.is_tensor(r0) else torch.device("cuda", torch.cuda.current_device())
    lo, hi = trim_length, len(frames) - trim_length
    written = 0
    for a in range(lo, hi, chunk):
        b = min(a + chunk, hi)
        part, cols, prio = _clip_tracks(tracks, a, b, colors, priority)
        if not part:
            # nobody here: one row of non-finite vertices draws nothing (include/hmmr_hip.h), so alpha is 0 everywhere
            nv = mesh_faces.max_index + 1
            part = [({"cams": torch.ones((1, 3), device=device), "verts": torch.full((1, nv, 3), float("nan"), device=device)},
                     None, (0, 1), [{"start_pt": [0, 0], "scale": 1.0, "im_shape": [IMG_SIZE, IMG_SIZE]}])]
            cols, prio = ['blue'], [None]
        out = video.render_scene(part, frames[a:b], mesh_faces, max_img_size=max_img_size, colors=cols, priority=prio,
                                 device=device).cpu().numpy()
        for j in range(a, b):
            Image.fromarray(out[j - a]).save(os.path.join(output_path, 'frame{:06d}.png'.format(j - trim_length)))
            written += 1
    print('Converting them to video..')
    made = make_video(vid_path, output_path)
    result = {"frames": output_path, "n_frames": written, "video": None, "note": None}
    if made is None:
        result["note"] = "no ffmpeg on PATH: the PNG frames are left in %s" % output_path
    elif made:
        result["video"] = vid_path
    else:
        result["note"] = "ffmpeg failed: the PNG frames are left in %s" % output_path
    return result


def render_person_clips(output_path, tracks, frames, faces=None, face_path='src/tf_smpl/smpl_faces.npy', chunk=64, degs=(0, 90), margin=10,
                        max_img_size=300, background=True, colors=None, device=None):
    """One person-centred clip per track of a video:

        output_path/track%02d/frame%06d.png   the views of `degs` side by side, each (h', w') of the track's video-level box
        output_path/track%02d.mp4             where an ffmpeg is installed

    tracks: per track (records_or_dict, layout, (start, end), image_og_params), as util/render/video.render_person_clips takes
    them; frames: uint8 [F,H,W,3], host or device.  The boxes and the cameras relative to them come from ONE hmmr_video_bbox call
    over the whole tracks (a box is a property of the whole video); each track is then rendered `chunk` frames at a time and
    comes to the host as finished uint8 frames.  Frame j of a track's folder is frame start + j of the video.
    degs / margin / max_img_size / background / colors: as video.render_person_clips (the deg == 0 view over the frames' window
    is this project's addition; the reference renders on white).  A track that cannot be rendered (an empty or non-finite
    track, a box without area or beyond the rasteriser's sizes) is named in a warning and in its entry, and skipped.
    Returns a list with one dict per track: 'frames' (the folder, None for a skipped track), 'n_frames' written, 'bbox',
    'status', 'size', and `video`: the mp4 path, or None with `note` saying that the mp4 exists already ("Video already
    exists!": nothing is rendered for that track), that no ffmpeg was found (or that it failed) and the PNG frames were left
    in place, or why the track was skipped."""
    import warnings
    from PIL import Image
    from ..util.render import person_view, video
    from ..util.render.nmr_renderer import load_faces
    from ..util.render.raster import MeshFaces, scene_color
    if not os.path.exists(output_path):
        os.mkdir(output_path)
    mesh_faces = faces if isinstance(faces, MeshFaces) else MeshFaces(faces if faces is not None else load_faces(face_path))
    if device is None:
        r0 = tracks[0][0]
        r0 = r0['cams'] if isinstance(r0, dict) else r0
        device = r0.device if torch.is_tensor(r0) and r0.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    frame_hw = tuple(frames.shape[1:3])
    video.check_track_ranges(tracks, len(frames))
    bbox, crops, status = video.video_bboxes(tracks, frame_hw, margin, device=device)
    results = []
    for t, (records, layout, (start, end), params) in enumerate(tracks):
        h, w, S = person_view.clip_size(bbox[t], max_img_size)
        folder, vid_path = os.path.join(output_path, 'track%02d' % t), os.path.join(output_path, 'track%02d.mp4' % t)
        res = {"frames": None, "n_frames": 0, "bbox": [int(x) for x in bbox[t]], "status": int(status[t]), "size": (h, w, S), "video": None,
               "note": None}
        results.append(res)
        why = video.clip_skip_reason(bbox[t], int(status[t]), (h, w, S))
        if why:
            res["note"] = "not rendered: %s" % why
            warnings.warn("render_person_clips: track %d is not rendered (%s, box %s)" % (t, why, res["bbox"]))
            continue
        if os.path.exists(vid_path):
            print('Video already exists!')
            res["note"] = "%s exists already" % vid_path
            continue
        if not os.path.exists(folder):
            os.mkdir(folder)
        res["frames"] = folder
        for a in range(0, end - start, chunk):
            b = min(a + chunk, end - start)
            rec = {k: records[k][a:b] for k in ('cams', 'verts')} if isinstance(records, dict) else records[a:b]
            _, verts = video._cams_verts(rec, layout, device)
            fr = None
            if background:
                fr = frames[start + a:start + b]
                fr = (fr if torch.is_tensor(fr) else torch.from_numpy(np.ascontiguousarray(fr))).to(device)
            views = video.person_clip_views(verts, crops[t][a:b], mesh_faces, bbox[t], (h, w, S), scene_color(t, colors), degs, fr)
            panels = [views[deg] for deg in degs]
            side = torch.cat(panels, dim=2).cpu().numpy()
            for j in range(a, b):
                Image.fromarray(side[j - a]).save(os.path.join(folder, 'frame{:06d}.png'.format(j)))
                res["n_frames"] += 1
        made = make_video(vid_path, folder)
        if made is None:
            res["note"] = "no ffmpeg on PATH: the PNG frames are left in %s" % folder
        elif made:
            res["video"] = vid_path
        else:
            res["note"] = "ffmpeg failed: the PNG frames are left in %s" % folder
    return results
