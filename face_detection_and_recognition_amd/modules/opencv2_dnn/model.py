"""The reference's OpenCV age / gender models (modules/opencv2_dnn/model.py) with the nets as one HIP plan (AgeGenderNet).

* OpenCVFaceAgeModel / OpenCVFaceGenderModel: the reference's constructors and ``__call__(cv2_img, pad_resize=False)``; the
  first argument is an AgeGenderNet (both nets; each model reads its own branch) where the reference takes a cv2.dnn.Net.
  They return the softmax probabilities (8,) / (2,) that ``net.forward()[0]`` returns in the reference.
* OpenCVFaceDetAgeGenderModel: any detector of this project (BlazeFaceModel, YOLOV5FaceModel: ``__call__`` -> rows
  [x1, y1, x2, y2, ..., conf] normalised to its input size) + the age / gender nets -> (dets, opt_labels) with the reference's
  labels f"{gender}:{p:.2f},{age}:{p:.2f}".  The reference's own Res10-SSD detector is not part of this project.
"""
from typing import List, Tuple

import numpy as np
import torch

from ..age_gender.age_gender_net import (AGE_LIST, GENDER_LIST, MEAN_BGR, AgeGenderNet, attr_crop_items_host, labels,
                                         run_on_items)
from ..models.base import Model
from ..utils.image import pad_resize_image, scale_coords


def _check_net(net, input_size, mean):
    if not isinstance(net, AgeGenderNet):
        raise TypeError(f"expected an AgeGenderNet, got {type(net).__name__}")
    if tuple(input_size) != tuple(net.input_size):
        raise ValueError(f"the nets take {net.input_size}, got INPUT_SIZE = {tuple(input_size)}")
    if not np.allclose(mean, MEAN_BGR, rtol=0, atol=1e-9):
        raise ValueError(f"the plan folds the mean {MEAN_BGR} into conv1; got {tuple(mean)}")


def _run_whole(net, cv2_img):
    """Both nets on the whole BGR image resized to 227 x 227 (blobFromImage's cv2.resize) -> host (age (8,), gender (2,))."""
    dev = net._device()
    h, w = cv2_img.shape[:2]
    frames = torch.from_numpy(np.ascontiguousarray(cv2_img)).to(dev).unsqueeze(0)
    items = torch.tensor([[0, 0, 0, w, h, 0, 0, net.input_size[0], net.input_size[1]]], dtype=torch.int32, device=dev)
    age, gender = run_on_items(net, frames, items, 1)
    return age[0].cpu().numpy(), gender[0].cpu().numpy()


class OpenCVFaceAgeModel(Model):
    __slots__ = ["age_net", "age_mean_values"]

    def __init__(self, age_net: AgeGenderNet, det_thres: float, bbox_area_thres: float,
                 INPUT_SIZE: Tuple[int, int] = (227, 227),
                 AGE_MEAN_VALUES: Tuple[float, float, float] = MEAN_BGR):
        """Predicts age groups ['(0-2)', '(4-6)', '(8-12)', '(15-20)', '(25-32)', '(38-43)', '(48-53)', '(60-100)']"""
        Model.__init__(self, INPUT_SIZE, det_thres, bbox_area_thres)
        _check_net(age_net, INPUT_SIZE, AGE_MEAN_VALUES)
        self.age_net = age_net
        self.age_mean_values = AGE_MEAN_VALUES

    def __call__(self, cv2_img: np.ndarray, pad_resize: bool = False) -> np.ndarray:
        if pad_resize:
            cv2_img = pad_resize_image(cv2_img, new_size=self.input_size, device=self.age_net._device())
        return _run_whole(self.age_net, cv2_img)[0]


class OpenCVFaceGenderModel(Model):
    __slots__ = ["gender_net", "gender_mean_values"]

    def __init__(self, gender_net: AgeGenderNet, det_thres: float, bbox_area_thres: float,
                 INPUT_SIZE: Tuple[int, int] = (227, 227),
                 GENDER_MEAN_VALUES: Tuple[float, float, float] = MEAN_BGR):
        """Predicts two genders ["Male", "Female"]"""
        Model.__init__(self, INPUT_SIZE, det_thres, bbox_area_thres)
        _check_net(gender_net, INPUT_SIZE, GENDER_MEAN_VALUES)
        self.gender_net = gender_net
        self.gender_mean_values = GENDER_MEAN_VALUES

    def __call__(self, cv2_img: np.ndarray, pad_resize: bool = False) -> np.ndarray:
        if pad_resize:
            cv2_img = pad_resize_image(cv2_img, new_size=self.input_size, device=self.gender_net._device())
        return _run_whole(self.gender_net, cv2_img)[1]


class OpenCVFaceDetAgeGenderModel(Model):
    """detector (a Model of this project) + AgeGenderNet -> ``__call__(cv2_img)`` = (dets above det_thres, opt_labels)."""

    __slots__ = ["face_net", "age_gender_net", "age_list", "gender_list"]

    def __init__(self, face_net: Model, age_gender_net: AgeGenderNet, det_thres: float = None, bbox_area_thres: float = None):
        det_thres = face_net.det_thres if det_thres is None else det_thres
        bbox_area_thres = face_net.bbox_area_thres if bbox_area_thres is None else bbox_area_thres
        Model.__init__(self, face_net.input_size, det_thres, bbox_area_thres, returns_opt_labels=True)
        _check_net(age_gender_net, age_gender_net.input_size, MEAN_BGR)
        self.face_net = face_net
        self.age_gender_net = age_gender_net
        self.age_list = list(AGE_LIST)
        self.gender_list = list(GENDER_LIST)

    def attributes(self, cv2_img: np.ndarray, face_dets: np.ndarray):
        """(age (k, 8), gender (k, 2)) host probabilities of the faces of rows face_dets (already thresholded); NaN rows
        for crops that come out empty (the reference's cv2.resize would raise on them)."""
        h, w = cv2_img.shape[:2]
        mw, mh = self.input_size
        k = len(face_dets)
        if k == 0:
            return np.zeros((0, len(AGE_LIST)), np.float32), np.zeros((0, len(GENDER_LIST)), np.float32)
        bboxes = face_dets[:, :4] * np.array([mw, mh, mw, mh])
        bboxes = scale_coords((mh, mw), bboxes, (h, w)).round()
        info = np.zeros((k, 5), np.float32)
        info[:, 1:5] = bboxes
        items_h = attr_crop_items_host(info, [(h, w)], dst=self.age_gender_net.input_size)
        net = self.age_gender_net
        dev = net._device()
        frames = torch.from_numpy(np.ascontiguousarray(cv2_img)).to(dev).unsqueeze(0)
        items = torch.from_numpy(items_h).to(dev)
        age, gender = run_on_items(net, frames, items, k)
        age, gender = age.cpu().numpy().copy(), gender.cpu().numpy().copy()
        empty = items_h[:, 7] == 0
        age[empty] = np.nan
        gender[empty] = np.nan
        return age, gender

    def __call__(self, cv2_img: np.ndarray) -> Tuple[np.ndarray, List[str]]:
        """Returns a tuple of face dets and age_gender pred txt labels"""
        face_dets = self.face_net(cv2_img)
        face_dets = face_dets[face_dets[:, -1] > self.det_thres]
        age, gender = self.attributes(cv2_img, face_dets)
        return face_dets, labels(age, gender)
