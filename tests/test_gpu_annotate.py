"""The annotated tracking video on the device: the Motion-JPEG encoder (`vbs_jpeg_encode`) against Pillow byte for byte,
the overlay (`vbs_draw_tracking`) against the sequential OpenCV restatement tests/helpers/cv_draw.py pixel for pixel, and
`MarkerTracker(..., write_video=True)` end to end on every input path."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")

import vbs_amd.synth as S                                     # noqa: E402
from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cv_draw  # noqa: E402

CROP = (1 / 8, 1 / 8, 1 / 16, 0)


def _pillow_jpeg(bgr, q):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, "JPEG", quality=q)
    return b.getvalue()


def _frames_of(w, h, seed):
    """Three different frames: synthetic markers, uniform noise, a flat frame with a saturated block."""
    rng = np.random.default_rng(seed)
    if min(w, h) >= 200:
        n = min(7, min(w, h) // 70)
        pitch = min(w, h) // (n + 1)
        synth = S.make_frames(S.grid_spec(w, h, n, pitch, pitch // 3), [1], seed=seed, channels=3)[0]
    else:                                                                    # (too small for a marker grid: a gradient)
        yy, xx = np.mgrid[0:h, 0:w]
        synth = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) % 256], axis=2).astype(np.uint8)
    flat = np.full((h, w, 3), 200, np.uint8)
    flat[h // 3:, : w // 2] = (255, 0, 40)
    return np.stack([synth, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), flat])


@pytest.mark.parametrize("w,h", [(480, 450), (640, 480), (1280, 1024), (333, 217), (17, 9)])
def test_jpeg_encoder_bytes_equal_pillow(w, h):
    from vbs_amd.video_io import MjpegDeviceEncoder
    frames = _frames_of(w, h, seed=w + h)
    # the encoder reads a strided crop view like the tracker's: frames embedded in a larger buffer
    big = torch.zeros((3, h + 3, w + 5, 3), dtype=torch.uint8, device="cuda")
    big[:, 2:2 + h, 3:3 + w] = torch.from_numpy(frames).cuda()
    view = big[:, 2:2 + h, 3:3 + w]
    for q in (50, 75, 95, 100):
        enc = MjpegDeviceEncoder("cuda:0", w, h, batch=4, quality=q)
        files = enc.fetch(enc.encode(view))
        assert len(files) == 3
        for i, f in enumerate(files):
            assert f == _pillow_jpeg(frames[i], q), (w, h, q, i)
            assert len(f) <= enc.frame_bound
        assert enc.downloaded_bytes == sum(map(len, files)) + 4 * 3
    # the bound is not only respected by compressible frames: noise at quality 100 fills more than half a byte per pixel
    assert len(files[1]) > w * h // 2 or w * h < 1000


def _overlay_case(h, w, m, n, seed):
    """det / table / ref_xy for n frames of m slots: markers within a few px of every border, overlapping ones, dropped
    (flag clear) ones; frame 0 has O == C."""
    rng = np.random.default_rng(seed)
    ref = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m)], axis=1)
    ref[:8] = [[1.2, 1.7], [w - 1.4, 2.2], [3.1, h - 0.6], [w - 2.6, h - 2.9], [w / 2, 0.3], [0.4, h / 2], [w - 0.2, h / 3],
               [w / 3, h - 0.1]]
    ref[8:12] = ref[12:16] + rng.uniform(-3, 3, (4, 2))                       # overlapping markers
    maxm = m + 4
    det = np.zeros((n, maxm, 6))
    table = np.zeros((n, m, 10), np.float32)
    for f in range(n):
        perm = rng.permutation(maxm)[:m]                                      # detection rows in another order than slots
        cur = ref + (0 if f == 0 else rng.uniform(-12, 12, (m, 2)))
        det[f, perm, 0:2] = cur
        det[f, perm, 2] = rng.uniform(8, 30, m)
        det[f, perm, 3] = det[f, perm, 2] * rng.uniform(0.5, 1.0, m)
        det[f, perm, 4] = rng.uniform(-180, 180, m)
        table[f, :, 0] = (rng.uniform(size=m) > 0.15) * 1 + 2 * (rng.uniform(size=m) > 0.5)
        table[f, :, 9] = perm
    return ref, det, table


@pytest.mark.parametrize("h,w,m", [(450, 480, 60), (131, 203, 25)])
def test_draw_tracking_equals_cv_draw(h, w, m):
    from vbs_amd.engine import Engine
    ref, det, table = _overlay_case(h, w, m, n=4, seed=h)
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (4, h + 4, w + 6, 3), dtype=np.uint8)
    eng = Engine(h, w, max_markers=det.shape[1], max_batch=4, device=0)
    ft = torch.from_numpy(frames).cuda()[:, 1:1 + h, 2:2 + w]                 # a crop view
    before = ft.clone()
    out = eng.draw_tracking(ft, torch.from_numpy(det).cuda(), torch.from_numpy(table).cuda(), ref).cpu().numpy()
    assert torch.equal(ft, before)
    for f in range(4):
        rows = [(ref[s, 0], ref[s, 1], *det[f, int(table[f, s, 9]), :5]) for s in range(m) if int(table[f, s, 0]) & 1]
        want = cv_draw.draw_frame(frames[f, 1:1 + h, 2:2 + w], rows)
        assert np.array_equal(out[f], want), (f, int((out[f] != want).any(-1).sum()))
    eng.close()


def _clip(tmp_path, n=6, seed=3):
    from vbs_amd.video_io import write_avi
    spec = S.config1()                                                       # 640 x 480, the reference's camera frame
    frames = S.make_frames(spec, range(n), seed=seed, channels=3)
    path = str(tmp_path / "clip.avi")
    write_avi(path, frames, fps=25.0, codec="MJPG", quality=90)
    return path, frames


def _decoded(path):
    from vbs_amd.video_io import AviReader
    r = AviReader(path)
    return np.stack([r.read()[1] for _ in range(len(r._frames))])


def _check_video(out_avi, csv_path, crops, q=95, fps=None):
    import pandas as pd
    from vbs_amd.video_io import AviReader
    r = AviReader(out_avi)
    assert r.isOpened() and len(r._frames) == len(crops)
    assert (r.width, r.height) == (crops.shape[2], crops.shape[1])
    if fps is not None:
        assert abs(r.fps - fps) < 1e-6
    df = pd.read_csv(csv_path, float_precision="round_trip")
    cols = ["Ox", "Oy", "Cx", "Cy", "major_axis", "minor_axis", "angle"]
    for i, (off, size) in enumerate(r._frames):
        rows = df[df.frameno == i][cols].to_numpy(dtype=np.float64)
        assert len(rows) > 0
        want = _pillow_jpeg(cv_draw.draw_frame(crops[i], [tuple(x) for x in rows]), q)
        assert bytes(r._buf[off:off + size]) == want, i
    ok, fr = r.read()                                                        # and the files decode
    assert ok and fr.shape == crops.shape[1:]


@pytest.mark.parametrize("id_mode", ["as_written", "full"])
def test_process_writes_the_tracked_video(tmp_path, id_mode):
    from vbs_amd.marker_detection import MarkerTracker, _crop_box
    try:
        import cv2  # noqa: F401
        pytest.skip("OpenCV present: VideoCapture is used, as in the reference")
    except ImportError:
        pass
    path, _ = _clip(tmp_path)
    dec = _decoded(path)
    l, r, t, b = _crop_box(640, 480, CROP)
    crops = dec[:, t:b, l:r]
    cfg = {"video_path": path, "crop_ratios": CROP, "num_layers": 5, "min_marker_distance": 20, "id_mode": id_mode, "batch": 4}
    plain = MarkerTracker({**cfg, "output_dir": str(tmp_path / "plain")})
    plain.process()
    assert not os.path.exists(plain.output_video)
    for sub, extra in (("dev", {}), ("pil", {"mjpeg_on_device": False})):
        t1 = MarkerTracker({**cfg, **extra, "output_dir": str(tmp_path / sub), "write_video": True})
        t1.process()
        assert t1.decode_path == ("device" if sub == "dev" else "pillow")
        assert open(t1.output_csv, "rb").read() == open(plain.output_csv, "rb").read()
        _check_video(t1.output_video, t1.output_csv, crops, fps=25.0)


def test_process_frames_npy_and_calibration_write_the_tracked_video(tmp_path):
    from vbs_amd.marker_detection import MarkerTracker, _crop_box
    path, frames = _clip(tmp_path, n=5, seed=4)
    l, r, t, b = _crop_box(640, 480, CROP)
    # process() on an .npy array (no "fps": 30 frames/s), quality from the config
    np.save(tmp_path / "arr.npy", frames)
    t0 = MarkerTracker({"video_path": str(tmp_path / "arr.npy"), "output_dir": str(tmp_path / "npy"), "crop_ratios": CROP,
                        "write_video": True, "video_quality": 80, "batch": 2, "id_mode": "full"})
    t0.process()
    _check_video(t0.output_video, t0.output_csv, frames[:, t:b, l:r], q=80, fps=30.0)
    # process_frames() on a device tensor, with calibration_params: the video shows the undistorted crop
    K = [[520.0, 0, 240.0], [0, 520.0, 225.0], [0, 0, 1]]
    calib = {"camera_matrix": K, "dist_coeffs": [0.04, -0.01, 0.0, 0.0, 0.0]}
    cfg = {"video_path": path, "output_dir": str(tmp_path / "cal"), "crop_ratios": CROP, "calibration_params": calib,
           "batch": 3}
    t1 = MarkerTracker({**cfg, "write_video": True})
    rows = t1.process_frames(torch.from_numpy(frames).cuda())
    t1._save_results(rows)
    t2 = MarkerTracker({**cfg, "output_dir": str(tmp_path / "cal2")})
    t2._save_results(t2.process_frames(torch.from_numpy(frames).cuda()))
    assert open(t1.output_csv, "rb").read() == open(t2.output_csv, "rb").read()
    und = np.stack([t1._undistort_frame(f[t:b, l:r]) for f in frames])
    _check_video(t1.output_video, t1.output_csv, und)


def test_write_video_errors(tmp_path):
    from vbs_amd.marker_detection import MarkerTracker
    from vbs_amd.video_io import AviReader
    gray = S.make_frames(S.config1(), range(2), seed=0)
    np.save(tmp_path / "g.npy", gray)
    with pytest.raises(ValueError, match="BGR"):
        MarkerTracker({"video_path": str(tmp_path / "g.npy"), "output_dir": str(tmp_path / "g"), "crop_ratios": (0, 0, 0, 0),
                       "write_video": True}).process()
    # a frame the workspace cannot hold, mid-clip: the video keeps the frames of the batches before it, and is readable
    spec = S.config2()
    frames = S.make_frames(spec, range(6), seed=2, channels=3)
    frames[4] = S.make_frames(S.grid_spec(spec.width, spec.height, 33, 30, 14, name="dense"), [1], seed=0, channels=3)[0]
    np.save(tmp_path / "clip.npy", frames)
    trk = MarkerTracker({"video_path": str(tmp_path / "clip.npy"), "output_dir": str(tmp_path / "o"),
                         "crop_ratios": (0, 0, 0, 0), "id_mode": "full", "batch": 2, "write_video": True})
    with pytest.raises(L.VbsError, match="frame 4"):
        trk.process()
    import pandas as pd
    done = int(pd.read_csv(trk.output_csv).frameno.max()) + 1
    r = AviReader(trk.output_video)
    assert r.isOpened() and 1 <= len(r._frames) == done < 6
    for _ in range(done):
        ok, fr = r.read()
        assert ok and fr.shape == frames.shape[1:]
