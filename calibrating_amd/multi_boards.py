"""A camera calibrated from pictures that show several boards each (the reference's calibrating/multi_boards.py:78-163).

``MultiBoards`` -- the boards as one target -- lives in ``boards``; ``MultiBoardsCam`` is the camera.  Every (image, board)
pair with enough corners is a frame of its own, keyed ``"{img}~{board}"``.  The reference detects board by board, image
by image; here the whole recording goes through ONE batched detection (``MultiBoards.find_image_points_batch``:
``imgproc.find_charuco_boards`` and ``corner_sub_pix`` on the GPU) where the boards form a set, and the calibration
through ``Cam.calibrate`` (``calibrate.calibrate_camera``).  Images are arrays; paths are not read here.
"""
import functools
from collections import defaultdict

import numpy as np

from .boards import MultiBoards
from .camera import Cam
from .geometry import mean_Ts
from .reconstruction_with_board import convert_cam_to_nerf_json

SEPARATOR = "~"


def _records_by_board(cam):
    """board name -> {image name: record}"""
    by_board = defaultdict(dict)
    for key, d in cam.items():
        img_name, board_name = key.split(SEPARATOR)
        by_board[board_name][img_name] = d
    return by_board


class MultiBoardsCam(Cam):
    """Cam class that supports several calibration boards in one image; each record's key is ``{img_key}~{board_key}``."""

    def __init__(self, images=None, boards=None, name=None, undistorted=False, calibrate_flags=0):
        """``images``: a dict key -> image or a sequence (keys "0", "1", ...), (h, w) or (h, w, 3) uint8 of one size, NumPy
        or CUDA.  ``boards``: a dict name -> board or a list (names "0", "1", ...).  Boards that form a set
        (``boards.MultiBoards``) are detected in one batched pass over the whole recording; another mix goes board by
        board, image by image.  Every (image, board) that shows at least 11 corners becomes the record
        ``self["{img}~{board}"]`` (``ids``, ``image_points``, ``object_points``, ``board``, ``img``); then ``calibrate()``."""
        super().__init__()
        if images is None:
            return
        if not isinstance(boards, dict):
            boards = dict((str(i), v) for i, v in enumerate(boards))
        if not isinstance(images, dict):
            if isinstance(images, str):
                images = [images]
            images = dict((str(i), v) for i, v in enumerate(images))
        for key, img in images.items():
            if isinstance(img, str):
                raise ValueError("MultiBoardsCam: images are not read from paths here -- load %r and pass the array" % (img,))
        for key in list(images) + list(boards):
            if not isinstance(key, str) or SEPARATOR in key:
                raise ValueError("MultiBoardsCam: image and board names are strings without %r, got %r" % (SEPARATOR, key))
        if not images or not boards:
            raise ValueError("MultiBoardsCam: no images or no boards")
        first = next(iter(images.values()))
        self.xy, self.name = (int(first.shape[1]), int(first.shape[0])), name
        self.undistorted, self.calibrate_flags = bool(undistorted), int(calibrate_flags)
        names, multi = list(boards), MultiBoards([boards[k] for k in boards])
        if multi.first_ids is not None:
            if isinstance(first, np.ndarray):
                batch = np.stack(list(images.values()))
            else:
                import torch
                batch = torch.stack(list(images.values()))
            seen, corners = multi.find_image_points_batch(batch)
            if not isinstance(seen, np.ndarray):
                seen, corners = seen.cpu().numpy(), corners.cpu().numpy()
            for k, img_key in enumerate(images):
                for b, board_name in enumerate(names):
                    frames = boards[board_name].to_frames(seen[k:k + 1, b], corners[k:k + 1, b])
                    if 0 in frames:
                        self[img_key + SEPARATOR + board_name] = dict(frames[0], board=boards[board_name], img=images[img_key])
        else:
            for img_key, img in images.items():
                for board_name, board in boards.items():
                    d = dict(img=img)
                    board.find_image_points(d)
                    if "image_points" in d:
                        self[img_key + SEPARATOR + board_name] = dict(d, board=board)
        self.calibrate()
        self.boards = boards

    def get_board_name_to_T_world(self, origin_to_center=False):
        """multi_boards.py:107-135: name -> the board's pose in board 0 (the first of ``boards``) -- over the images that
        show both with a pose, ``inv(T_board0) @ T_board`` averaged by ``mean_Ts``, the images in sorted order (the
        reference walks a set of names, whose order Python does not fix; ``mean_Ts`` depends on it in the last bits).
        ``origin_to_center``: the poses relative to their own mean instead of board 0."""
        boards = self.boards
        board_name_to_img_names = _records_by_board(self)
        board_name0 = list(boards)[0]
        board_name_to_T_world = board_name_to_T_board_in_board0 = {}
        for board_name in boards:
            ds0 = board_name_to_img_names[board_name0]
            ds = board_name_to_img_names[board_name]
            Ts = []
            for img_name in sorted(set(ds).intersection(ds0)):
                if "T" in ds[img_name] and "T" in ds0[img_name]:
                    Ts.append(np.linalg.inv(ds0[img_name]["T"]) @ ds[img_name]["T"])
            assert Ts, f"{board_name} has common vision with first board: {board_name0}"
            board_name_to_T_board_in_board0[board_name] = mean_Ts(Ts)
        if origin_to_center:
            to_T_world = np.linalg.inv(mean_Ts(list(board_name_to_T_board_in_board0.values())))
            board_name_to_T_world = {n: to_T_world @ T for n, T in board_name_to_T_board_in_board0.items()}
        return board_name_to_T_world

    def images_in_world(self):
        """image name -> a copy of one of its records (board 0's where it shows board 0) with ``T_cam_in_world``: the mean
        over the boards the image shows of ``T_world_board @ inv(T_board_in_cam)``, the world being
        ``get_board_name_to_T_world(True)``'s (multi_boards.py:139-159; an image that does not show board 0 is kept, where
        the reference fails on it)."""
        board_name_to_T_world = self.get_board_name_to_T_world(True)
        board_name_to_img_names = _records_by_board(self)
        ds_new = {}
        for board_name in self.boards:
            for img_name, d in board_name_to_img_names[board_name].items():
                if "T" in d:
                    ds_new.setdefault(img_name, dict(d))
        for img_name in ds_new:
            T_cam_in_worlds = [board_name_to_T_world[board_name] @ np.linalg.inv(board_name_to_img_names[board_name][img_name]["T"])
                               for board_name in self.boards if "T" in board_name_to_img_names[board_name].get(img_name, "")]
            ds_new[img_name]["T_cam_in_world"] = mean_Ts(T_cam_in_worlds)
        return ds_new

    @functools.wraps(convert_cam_to_nerf_json)
    def convert_to_nerf_json(self, *args, **argkws):
        cam_new = self.copy()
        cam_new.update(self.images_in_world())
        return convert_cam_to_nerf_json(cam_new, *args, **argkws)
