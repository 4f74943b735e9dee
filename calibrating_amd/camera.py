"""``Cam``: the per-camera record ``Stereo`` needs -- K, D, xy, name.

Only the record format of the reference's ``Cam`` is mirrored (``Cam.load`` / ``Cam.dump``,
/root/reference/calibrating/camera.py:407-448): a YAML / dict record with either ``K`` (3x3) or
``fx, fy, cx, cy``, optional ``D`` (default five zeros), ``xy`` = (width, height) (required), and the
free-form keys ``name``, ``T_in_main_cam``, ``retval``.  Intrinsic calibration itself runs on the GPU from detected
points: ``Cam.from_detections(frames, xy).calibrate()`` (camera.py:63-93: cv2.calibrateCamera; csrc/calibrate.hip).
Detecting a board, caches and feature pictures stay with the caller.
Two point methods of the reference's ``Cam`` run on the GPU: ``undistort_points`` and ``project_points``
(camera.py:275-287; csrc/points.hip), the step between a matcher's raw pixels and the epipolar path.  So do its two
alignment pictures, ``vis_depth_alignment`` and ``vis_reproject_img_alignment`` (camera.py:311-342; csrc/vis.hip), and the
pose of a target from its detected points: ``perspective_n_point``, ``solve_poses`` for every stored frame in one launch,
``get_T_cam2_in_self`` (camera.py:266-273, 289-296; csrc/pnp.hip).  Detecting the points stays with the caller.
The board as ground truth: ``get_calibration_board_T``, ``get_calibration_board_depth`` and its batch form
(camera.py:214-264; csrc/hull.hip) give the dense depth of the board's plane in an image or a whole recording.
"""
import copy

import numpy as np
import yaml

_INTRINSIC_KEYS = ("fx", "fy", "cx", "cy")
_RECORD_KEYS = ("D", "xy", "name", "T_in_main_cam", "retval")  # what a dump carries besides the intrinsics


def intrinsic_format_conversion(K_or_dic):
    """K (3x3) <-> dict(fx, fy, cx, cy): the two spellings of the intrinsics in a camera record."""
    if isinstance(K_or_dic, dict):
        fx, fy, cx, cy = (K_or_dic[k] for k in _INTRINSIC_KEYS)
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    K = np.asarray(K_or_dic)
    return {k: float(v) for k, v in zip(_INTRINSIC_KEYS, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))}


def read_record(source):
    """A record from a dict (deep-copied), a YAML document (a string containing a newline) or a YAML file
    path -- the three input forms ``Cam.load`` / ``Stereo.load`` of the reference accept."""
    if isinstance(source, (dict, list)):
        return copy.deepcopy(source)
    if "\n" in source:
        return yaml.safe_load(source)
    with open(source) as f:
        return yaml.safe_load(f)


def write_record(record, path=""):
    """YAML text of ``record`` stamped with the package version; also written to ``path`` when given."""
    from .__info__ import __version__
    text = yaml.safe_dump(dict(record, _calibrating_version=__version__))
    if path:
        with open(path, "w") as f:
            f.write(text)
    return text


def _plain(value):
    if isinstance(value, np.ndarray):
        return value.tolist()
    return list(value) if isinstance(value, tuple) else value


class Cam(dict):
    def __init__(self, K=None, D=None, xy=None, name=None):
        super().__init__()
        if K is not None:
            self.K = np.float64(K)
            self.D = np.zeros((1, 5)) if D is None else np.float64(D)
            self.xy = tuple(xy)
            self.name = name

    @classmethod
    def init_by_K_D(cls, K, D=None, xy=None, name=None):
        return cls(K, D, xy, name)

    @classmethod
    def from_detections(cls, frames, xy, name=None, undistorted=False, calibrate_flags=0):
        """A camera that holds detections and no intrinsics yet: ``frames`` maps key -> ``dict(image_points=...,
        object_points=...)``, arrays or the reference's id -> array dicts (joined by ``geometry.join_points``).
        ``undistorted`` and ``calibrate_flags`` are the reference's constructor arguments (camera.py:32-43); ``calibrate()``
        makes K and D from them."""
        cam = cls()
        cam.xy, cam.name, cam.undistorted, cam.calibrate_flags = tuple(xy), name, bool(undistorted), int(calibrate_flags)
        for key, frame in frames.items():
            cam[key] = dict(frame)
        return cam

    def calibrate(self):
        """``cv2.calibrateCamera`` over every valid frame that holds object points (camera.py:63-93), on the GPU
        (``calibrate.calibrate_camera``): sets ``K``, ``D``, ``retval`` and, for every such key, ``self[key]["T"]`` and
        ``["reprojection_error"]``.  ``undistorted`` selects the reference's flag set (no lens: tangential and radial
        coefficients fixed at 0).  A frame left out of the joint problem gets no pose (and loses an earlier one).  A camera
        that cannot be calibrated raises ``ValueError`` and keeps what it had.  Returns ``self``."""
        from . import calibrate, geometry
        keys = sorted(k for k in self.valid_keys if "object_points" in self[k])
        if not keys:
            raise ValueError("No any valid image!")
        uvs = [np.asarray(geometry.join_points(self[k]["image_points"])).reshape(-1, 2) for k in keys]
        xyzs = [np.asarray(geometry.join_points(self[k]["object_points"])).reshape(-1, 3) for k in keys]
        for k, a, b in zip(keys, uvs, xyzs):
            if len(a) != len(b):
                raise ValueError("%r: %d image points and %d object points" % (k, len(a), len(b)))
        flags = calibrate.UNDISTORTED_FLAGS if getattr(self, "undistorted", False) else getattr(self, "calibrate_flags", 0)
        res = calibrate.calibrate_camera(np.concatenate(xyzs), np.concatenate(uvs), self.xy, counts=[len(a) for a in uvs], flags=flags)
        self.retval, self.K, self.D = res["retval"], res["K"], res["D"]
        for i, k in enumerate(keys):
            d = self[k]
            if res["status"][i] == 0:
                d["T"], d["reprojection_error"] = res["T"][i], float(res["reprojection_error"][i])
            else:
                d.pop("T", None)
                d.pop("reprojection_error", None)
        return self

    def load(self, path_or_str_or_dict=None):
        """``Cam.load(record)`` (called on the class: builds a new Cam) or ``cam.load(record)`` (in place)."""
        if path_or_str_or_dict is None:  # Cam.load(x) binds x to `self`
            return Cam().load(self)
        if isinstance(path_or_str_or_dict, Cam):
            return path_or_str_or_dict.copy()
        rec = read_record(path_or_str_or_dict)
        rec.pop("_calibrating_version", None)
        if "K" in rec:
            K = rec.pop("K")
        else:
            K = intrinsic_format_conversion({k: rec.pop(k) for k in _INTRINSIC_KEYS})
        xy = tuple(rec.pop("xy", getattr(self, "xy", ())))
        assert len(xy), "Need xy"
        self.K = np.float64(K)
        self.D = np.float64(rec.pop("D")) if "D" in rec else np.zeros((1, 5))
        self.xy = xy
        self.__dict__.update(rec)
        return self

    def copy(self):
        return type(self)().load(self.dump(return_dict=True))

    def dump(self, path="", return_dict=False):
        rec = {k: _plain(self.__dict__[k]) for k in _RECORD_KEYS if k in self.__dict__}
        rec.update(intrinsic_format_conversion(self.K))
        return rec if return_dict else write_record(rec, path)

    # intrinsics by name and the fields of view in DEGREES (reference camera.py:500-530; its boxx trig works in degrees)
    fx = property(lambda self: self.K[0, 0])
    fy = property(lambda self: self.K[1, 1])
    cx = property(lambda self: self.K[0, 2])
    cy = property(lambda self: self.K[1, 2])

    @property
    def fovs(self):
        half_x, half_y = self.xy[0] / 2 / self.fx, self.xy[1] / 2 / self.fy  # tangents of the half angles
        deg = lambda t: float(np.degrees(2 * np.arctan(t)))  # noqa: E731
        return dict(fov=deg(np.hypot(half_x, half_y)), fovx=deg(half_x), fovy=deg(half_y))

    def project_points(self, xyzs, T=None):
        """Pixels of this camera's RAW image for 3-D points (camera.py:275-280: cv2.projectPoints with K and D), on the
        GPU.  ``xyzs``: (n, 3) or (n, 1, 3), float32 or float64, ndarray or CUDA tensor -> (n, 2) of the same kind and
        type.  ``T``: the 4x4 pose that takes the points into this camera's frame; None = they are in it already.  The
        pose goes through cv2's two Rodrigues passes on the host (matrix -> vector -> matrix)."""
        from . import geometry, imgproc
        rvec, tvec = (np.zeros((3, 1)), np.zeros((3, 1))) if T is None else geometry.T_to_r_t(T)
        return imgproc.project_points(xyzs, rvec, tvec, self.K, self.D)

    def undistort_points(self, uvs, iters=5):
        """Pixels of the RAW image -> pixels of the undistorted (pinhole K) image (camera.py:282-287), on the GPU: what a
        matcher's or a flow's points need before ``EssentialMatrixStereo`` / ``ReconstructionExtrinsics`` see them.
        ``uvs``: (n, 2) or (n, 1, 2), float32 or float64, ndarray or CUDA tensor -> (n, 2) float64 of the same kind
        (float32 points come back as float64, as NumPy's promotion makes them in the reference).  ``iters``: rounds of
        cv2.undistortPoints' iteration (cv2 runs 5); more for strong lenses."""
        from . import imgproc
        return imgproc.undistort_points(uvs, self.K, self.D, iters=iters, pixels=True)

    # ---- poses from points (camera.py:148-149, 266-273, 289-296, 371-372; csrc/pnp.hip) ----
    @property
    def valid_keys(self):
        """The frames in which the target was seen: keys whose record holds at least one image point (or id)."""
        return {key for key, frame in self.items() if len(frame.get("image_points", ()))}

    def valid_keys_intersection(cam1, cam2):
        """The frames in which both cameras saw the target, sorted."""
        return sorted(cam1.valid_keys & cam2.valid_keys)

    def perspective_n_point_batch(self, image_points, object_points, counts=None, T0=None):
        """``pnp.solve_pnp_batch`` with this camera's K and D: the poses of one target in many frames, one launch."""
        from . import pnp
        return pnp.solve_pnp_batch(object_points, image_points, self.K, self.D, counts=counts, T0=T0)

    def perspective_n_point(self, image_points, object_points):
        """The pose of a target from its points (camera.py:266-273: cv2.solvePnPGeneric), on the GPU -> the reference's
        ``dict(T=(4, 4), retval=1, reprojection_error=...)``.  The points are (n, 2) / (n, 3) arrays or the reference's
        id -> points dicts, joined in sorted-key order.  ``T`` is the float64 pose itself (the reference rounds it through
        a float32 Rodrigues vector).  A frame that cannot be solved raises ``ValueError`` with its status."""
        from . import geometry, pnp
        image_points = geometry.join_points(image_points)
        object_points = geometry.join_points(object_points)
        if getattr(image_points, "ndim", 0) == 3 and image_points.shape[1] == 1:
            image_points = image_points[:, 0]
        res = self.perspective_n_point_batch(image_points[None], object_points[None])
        status = int(res["status"][0])
        if status != pnp.STATUS_OK:
            raise ValueError("perspective_n_point: status %d (%s)" % (status, pnp.STATUS_TEXT[status]))
        return dict(T=res["T"][0], retval=1, reprojection_error=res["reprojection_error"][0])

    def solve_poses(self):
        """``cam[key]["T"]`` and ``cam[key]["reprojection_error"]`` for every valid key whose record also holds
        ``object_points`` (a valid key without them is left alone), in ONE launch over all frames.  The stored points are
        host data -- ndarrays, or id -> ndarray dicts --, as the reference's detectors leave them; points on the GPU go
        through ``perspective_n_point_batch``.  Returns key -> status word; a frame whose status is not 0 gets no pose
        (and loses an earlier one)."""
        from . import geometry
        keys = sorted(k for k in self.valid_keys if "object_points" in self[k])
        if not keys:
            return {}
        uvs = [np.asarray(geometry.join_points(self[k]["image_points"])).reshape(-1, 2) for k in keys]
        xyzs = [np.asarray(geometry.join_points(self[k]["object_points"])).reshape(-1, 3) for k in keys]
        for k, a, b in zip(keys, uvs, xyzs):
            if len(a) != len(b):
                raise ValueError("%r: %d image points and %d object points" % (k, len(a), len(b)))
        res = self.perspective_n_point_batch(np.concatenate(uvs), np.concatenate(xyzs), counts=[len(a) for a in uvs])
        for i, k in enumerate(keys):
            d = self[k]
            if res["status"][i] == 0:
                d["T"], d["reprojection_error"] = res["T"][i], float(res["reprojection_error"][i])
            else:
                d.pop("T", None)
                d.pop("reprojection_error", None)
        return {k: int(s) for k, s in zip(keys, res["status"])}

    # ---- the board as ground truth (camera.py:214-264; csrc/hull.hip) ----
    def get_board(cam=None, d=None, board=None):
        """The board to look for: ``board`` > ``d["board"]`` > ``cam.board`` (camera.py:253-264)."""
        if board is None:
            if d and d.get("board"):
                board = d.get("board")
            elif hasattr(cam, "board"):
                board = cam.board
        assert board, "Please set board or cam.board"
        return board

    def get_calibration_board_T(self, img_or_d, board=None):
        """The record of one image with the board's pose in it (camera.py:214-232): ``board.find_image_points`` sets
        ``image_points`` / ``object_points``, ``perspective_n_point`` adds ``T``, ``retval``, ``reprojection_error``.
        ``img_or_d``: an image (ndarray or CUDA tensor) or a record with ``"img"``; a record is copied, not changed.  A
        board that is not found leaves the record without ``image_points`` and ``T``.  Paths are not read here."""
        if isinstance(img_or_d, dict):
            d = img_or_d.copy()
            if isinstance(d.get("img"), str) or "img" not in d:
                raise ValueError("get_calibration_board_T: images are not read from paths here -- load the image and pass it "
                                 "as d['img']")
        elif isinstance(img_or_d, str):
            raise ValueError("get_calibration_board_T: images are not read from paths here -- load %r and pass the array"
                             % (img_or_d,))
        else:
            d = dict(img=img_or_d)
        assert tuple(d["img"].shape[:2][::-1]) == tuple(self.xy)
        board = self.get_board(d, board)
        board.find_image_points(d)
        if "image_points" in d:
            d.update(self.perspective_n_point(d["image_points"], d["object_points"]))
        return d

    def _board_rows(self, T, object_points):
        """(f, n, 3) float64 CUDA rows (u, v, z) of the board's points in every frame, nearest last: ``object_points`` (n, 3)
        through each pose of ``T`` (f, 4, 4), then the pinhole projection with K -- D is ignored, the reference's quirk
        (``point_cloud_to_depth(xyz, K, xy)``).  Every product and sum is one elementwise float64 operation, left to
        right, so NumPy gives the same bits.  The order is the z-buffer's: farthest first, so the last row of a pixel is
        the nearest one."""
        import torch
        o = object_points.to(torch.float64)
        x, y, z = o[None, :, 0], o[None, :, 1], o[None, :, 2]
        cam = [T[:, i, 0, None] * x + T[:, i, 1, None] * y + T[:, i, 2, None] * z + T[:, i, 3, None] for i in range(3)]
        K = [[float(v) for v in row] for row in np.asarray(self.K, np.float64)[:3, :3]]
        p, q, s = (K[i][0] * cam[0] + K[i][1] * cam[1] + K[i][2] * cam[2] for i in range(3))
        rows = torch.stack([p / s, q / s, s], -1)
        order = torch.sort(-s, dim=1, stable=True).indices  # argsort(-z), ties in row order
        return torch.gather(rows, 1, order[:, :, None].expand(-1, -1, 3))

    def _board_depth(self, T, object_points, zero_frames, is_dense):
        """``point_cloud_to_depth`` of the board in every frame and, dense, ``1 / fill(1 / sparse)`` inside the hull."""
        import torch
        from . import sparse
        w, h = int(self.xy[0]), int(self.xy[1])
        rows = self._board_rows(T, object_points)
        frames = int(rows.shape[0])
        if is_dense:
            # what the scatter and 1 / sparse leave of a row: its pixel and its inverse depth; the last row of a pixel stays
            samples = torch.stack([torch.round(rows[..., 0]), torch.round(rows[..., 1]), 1 / rows[..., 2]], -1)
            return sparse.interpolate_uvzs_in_hull(samples, (h, w), reciprocal=True, keep_last_per_pixel=True, zero_frames=zero_frames)
        # the scatter of all frames at once: frame f is rows f h .. f h + h - 1 of one tall image; what leaves its frame is dropped
        u, v = torch.round(rows[..., 0]), torch.round(rows[..., 1])
        inside = (u >= 0) & (u < w) & (v >= 0) & (v < h) & ~zero_frames[:, None]
        nan = torch.full_like(u, float("nan"))
        v = v + torch.arange(frames, dtype=torch.float64, device=u.device)[:, None] * h
        uvz = torch.stack([torch.where(inside, u, nan), torch.where(inside, v, nan), rows[..., 2]], -1).reshape(-1, 3)
        return sparse.uvzs_to_arr2d(uvz, (frames * h, w)).reshape(frames, h, w)

    def get_calibration_board_depth(cam, img_or_d, is_dense=True, board=None):
        """The record of ``get_calibration_board_T`` with ``depth``, the depth of the board's plane as ground truth
        (camera.py:234-251), on the GPU: the object points through ``T``, the pinhole ``point_cloud_to_depth(xyz, K, xy)``
        (D is ignored: the reference's quirk, kept), and with ``is_dense`` ``1 / fill(1 / sparse)`` by
        ``sparse.interpolate_uvzs_in_hull`` -- float32, ``+inf`` outside the board's hull as in the reference; without
        ``is_dense`` the sparse float64 depth.  Where the board is not found: zeros.  An ndarray image gives an ndarray, a CUDA
        image a CUDA tensor."""
        import torch
        from ._arrays import is_np, to_caller, to_device
        d = cam.get_calibration_board_T(img_or_d, board=board)
        was_np = is_np(d["img"])
        if "object_points" not in d or "T" not in d:
            d["depth"] = np.zeros(cam.xy[::-1]) if was_np else torch.zeros(tuple(cam.xy[::-1]), dtype=torch.float64, device=d["img"].device)
            return d
        object_points = d["object_points"]
        if isinstance(object_points, dict):
            object_points = np.concatenate(list(object_points.values()), 0)
        if was_np:
            from . import _native
            _native.require_device()
        dev = torch.device("cuda", torch.cuda.current_device()) if was_np else d["img"].device
        T = torch.from_numpy(np.ascontiguousarray(d["T"], np.float64)[None]).to(dev)
        o = torch.from_numpy(np.ascontiguousarray(object_points)).to(dev)
        depth = cam._board_depth(T, o, torch.zeros(1, dtype=torch.bool, device=dev), is_dense)
        d["depth"] = to_caller(depth[0], was_np)
        return d

    def get_calibration_board_depth_batch(cam, images, board=None, is_dense=True):
        """``get_calibration_board_depth`` of a whole recording in one call -> ``dict(depth (f, h, w), T (f, 4, 4) float64,
        found (f,) bool, status (f,) int32)``, ndarrays for ndarray images and CUDA tensors for CUDA tensors.  ``images``:
        (f, h, w) gray or (f, h, w, 3).  ``board.find_image_points_batch`` detects and refines, ``perspective_n_point_batch``
        poses, one batched fill writes the depth: no frame is handled on the host, and nothing read back decides what is
        launched beyond the one planarity test of the pose solver.  A frame without a board, or whose pose is not
        solved, has ``found`` False, zeros for its depth and NaN in its ``T``; ``status`` is the pose solver's (0 ok).
        Frame i equals ``get_calibration_board_depth(images[i])`` bit for bit."""
        import torch
        from ._arrays import check_array, is_np, to_caller, to_device
        check_array(images, "images")
        if len(images.shape) not in (3, 4) or tuple(images.shape[1:3][::-1]) != tuple(cam.xy):
            raise ValueError("images must be (f, %d, %d) or (f, %d, %d, 3), got %s"
                             % (cam.xy[1], cam.xy[0], cam.xy[1], cam.xy[0], tuple(images.shape)))
        board = cam.get_board(None, board)
        was_np = is_np(images)
        imgs = to_device(images)
        seen, corners = board.find_image_points_batch(imgs)
        o = torch.from_numpy(np.ascontiguousarray(board.object_points)).to(imgs.device)
        res = cam.perspective_n_point_batch(corners, o)
        found = seen.to(torch.bool) & (res["status"] == 0)
        depth = cam._board_depth(res["T"], o, ~found, is_dense)
        return dict(zip(("depth", "T", "found", "status"), to_caller((depth, res["T"], found, res["status"]), was_np)))

    def _pose_keys(cam1, cam2):
        return [k for k in cam1.valid_keys_intersection(cam2) if "T" in cam1[k] and "T" in cam2[k]]

    def get_T_cam2_in_self(cam1, cam2):
        """The pose of ``cam2`` in this camera from the frames both have a pose for (camera.py:289-296): per common key
        ``cam1[key]["T"] @ inv(cam2[key]["T"])``, then ``geometry.mean_Ts``.  Host, float64."""
        from . import geometry
        return geometry.mean_Ts([cam1[key]["T"] @ np.linalg.inv(cam2[key]["T"]) for key in cam1._pose_keys(cam2)])

    def _resolve_T_cam2(cam1, cam2, T):
        if T is not None:
            return T
        if not (isinstance(cam2, Cam) and cam1._pose_keys(cam2)):
            raise NotImplementedError("pass T (cam2 in cam1): board-based extrinsics are outside the MI355X path")
        return cam1.get_T_cam2_in_self(cam2)

    def project_cam2_depth(cam1, cam2, depth2, T=None, interpolation=1.5):
        """Depth image of ``cam2`` re-projected into this camera (camera.py:298-309), on the GPU.
        ``T`` = pose of cam2 in this camera (4x4); None resolves through ``get_T_cam2_in_self`` when both cameras carry
        poses under a common key (``solve_poses``), and is refused otherwise: detecting a board is the caller's."""
        T = cam1._resolve_T_cam2(cam2, T)
        from . import pointcloud
        rate = pointcloud.get_appropriate_interpolation_rate(cam1, cam2, interpolation)
        return pointcloud.project_depth(depth2, cam2.K, T, cam1.K, cam1.xy, interpolation_rate=rate)

    def reproject_img(cam1, cam2, depth2, img2, T=None, interpolation=1.5):
        """``img2`` of ``cam2`` brought into this camera's frame through ``depth2`` -- the image half of
        ``vis_reproject_img_alignment`` (camera.py:322-342), on the GPU; ``Stereo.undistort_img`` gives the other half.
        ``T`` = pose of cam2 in this camera (4x4), required as in ``project_cam2_depth``."""
        assert not np.any(cam2.D), f"cam2.D has distort: {cam2.D}"
        T = cam1._resolve_T_cam2(cam2, T)
        from . import pointcloud
        rate = pointcloud.get_appropriate_interpolation_rate(cam1, cam2, interpolation)
        return pointcloud.reproject_img(img2, depth2, cam2.K, T, cam1.K, cam1.xy, interpolation_rate=rate)

    def undistort_img(self, img):
        """``cv2.undistort(img, K, D)`` of this camera's raw image on the GPU (uint8, ndarray or CUDA tensor)."""
        from . import imgproc
        from ._arrays import is_np, to_caller, to_device
        i = to_device(img)
        mxy, ma = imgproc.undistort_maps_device(self.K, self.D, self.xy, device=i.device)
        return to_caller(imgproc.remap_fixed_bilinear(i, mxy, ma), is_np(img))

    def vis_depth_alignment(self, img, depth):
        """Do ``img`` (raw, not undistorted) and ``depth`` line up? (camera.py:311-320), on the GPU: the undistorted image
        and the depth -- clipped to 5 m (5000 for uint16), divided by its maximum from a device reduction, * 255, through
        JET * 0.75 -- as the four tiles of ``vis.vis_align``.  A depth without a positive pixel is index 0 throughout."""
        from . import vis
        from ._arrays import is_np, to_caller, to_device
        n, h, w, batched, name = vis._plane(depth, "depth", vis._DEPTH_TYPES)
        if is_np(img) != is_np(depth):
            raise TypeError("img and depth must both be NumPy arrays or both be CUDA tensors")
        i = self.undistort_img(to_device(img))
        d = to_device(depth, device=i.device)
        table = vis._device_table(vis._jet_bgr_075(), d.device)
        pic = vis._depth_picture(d, name, n, h * w, table, clip=(0.0, 5000.0 if name == "uint16" else 5.0),
                                 range_mode=vis._RANGE_MAX, scale=255.0, zero_mask=False, what="vis_depth_alignment")
        tiles = vis.vis_align(i, pic.view(((n,) if batched else ()) + (h, w, 3)))
        return [to_caller(t, is_np(img)) for t in tiles]

    def vis_reproject_img_alignment(cam1, cam2, depth2, img2, img1, T=None, interpolation=1.5):
        """Does ``img2`` of ``cam2``, brought here through ``depth2``, line up with this camera's ``img1`` (both raw)?
        (camera.py:322-342), on the GPU: ``vis.vis_align(cam1.undistort_img(img1), cam1.reproject_img(...))``.  ``T`` = pose
        of cam2 in this camera, required as in ``project_cam2_depth``; a distorted ``cam2`` is refused."""
        from . import vis
        if np.any(cam2.D):
            raise ValueError(f"cam2.D has distort: {cam2.D}")
        T = cam1._resolve_T_cam2(cam2, T)
        return vis.vis_align(cam1.undistort_img(img1), cam1.reproject_img(cam2, depth2, img2, T, interpolation))
