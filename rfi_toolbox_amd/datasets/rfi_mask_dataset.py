"""RFIMaskDataset: the directory mode of the reference's dataset (datasets/rfi_mask_dataset.py), normalised on the GPU.

``data_dir`` holds one directory per sample with ``input.npy`` ((8, T, F) float64, as ``save_example_pair_npy``
writes it) and ``rfi_mask.npy``.  The samples are indexed in ``os.listdir`` order -- not sorted -- as the reference
indexes them.  All inputs are uploaded once as fp64; the dataset-wide statistics (``global_min``, ``global_max``,
``mean``, ``std``, and for ``robust_scale`` ``robust_median`` / ``robust_iqr``) and the transform run on the device
(``preprocessing.Normalizer``, scope "dataset").  ``__getitem__`` gives the reference's pair: a float32 (8, T, F)
tensor and a float32 (1, T, F) mask tensor, through ``transform`` if given.

Beyond the reference: ``.images`` (host float32 (N, T, F, 8)) and ``.labels`` (uint8 (N, T, F), non-zero mask), which
is what ``training.train_rfi_model`` / ``evaluate_rfi_model`` take, and ``device_images()`` / ``device_labels()``, the
same two arrays in HBM.  The measurement-set mode needs CASA and is not provided.
"""
from __future__ import annotations

import os

import numpy as np
import torch

__all__ = ["RFIMaskDataset"]


class RFIMaskDataset:
    def __init__(self, data_dir, transform=None, normalization="global_min_max", use_ms=False, ms_name=None,
                 field_selection=None, device=None):
        from ..preprocessing.normalization import METHODS
        self.data_dir = data_dir
        self.transform = transform
        self.normalization = normalization
        self.use_ms = use_ms
        self.ms_name = ms_name
        self.field_selection = field_selection
        self.device = device
        self.global_min = np.inf
        self.global_max = -np.inf
        self.mean = self.std = self.robust_median = self.robust_iqr = None
        self.sample_dirs = []
        if use_ms:
            if not ms_name:
                raise ValueError("ms_name must be provided when use_ms is True")
            raise ImportError("CASA is required for use_ms=True but is not installed.\n"
                              "Install with: pip install rfi-toolbox[casa]")
        if normalization not in METHODS:
            raise ValueError(f"Unsupported normalization method: {normalization}")
        self.sample_dirs = [os.path.join(data_dir, d) for d in os.listdir(data_dir)
                            if os.path.isdir(os.path.join(data_dir, d))]
        if not self.sample_dirs:
            raise ValueError(f"no sample directories in {data_dir}")
        inputs = [np.load(os.path.join(d, "input.npy")) for d in self.sample_dirs]
        masks = [np.load(os.path.join(d, "rfi_mask.npy")) for d in self.sample_dirs]
        for d, x, m in zip(self.sample_dirs, inputs, masks):
            if x.ndim != 3 or x.shape[0] != 8 or x.shape != inputs[0].shape:
                raise ValueError(f"{d}/input.npy: expected (8, T, F) of one size, got {x.shape}")
            if m.shape != x.shape[1:]:
                raise ValueError(f"{d}/rfi_mask.npy: expected {x.shape[1:]}, got {m.shape}")
        self.masks = np.stack(masks).astype(np.float32)                  # __getitem__'s mask values
        self.labels = np.ascontiguousarray((self.masks != 0).astype(np.uint8))
        self._calculate_normalization_params(np.stack(inputs).astype(np.float64, copy=False))

    def _calculate_normalization_params(self, stack):
        from ..preprocessing.normalization import Normalizer
        from ..runtime import Context
        ctx = Context.get(self.device)
        raw = ctx.to_device(stack)                                       # (N, 8, T, F) fp64, uploaded once
        self.normalizer = Normalizer(self.normalization, scope="dataset", device=self.device).fit(raw)
        for k in ("global_min", "global_max", "mean", "std", "robust_median", "robust_iqr"):
            setattr(self, k, getattr(self.normalizer, k))
        self._images_dev = self.normalizer.transform(raw, out="nhwc")
        self._labels_dev = None
        self.images = self._images_dev.numpy()                           # (waits for the transform; `raw` may go)

    def device_images(self):
        """The normalised inputs in HBM: DeviceArray float32 (N, T, F, 8)."""
        return self._images_dev

    def device_labels(self):
        """The labels in HBM: DeviceArray uint8 (N, T, F)."""
        if self._labels_dev is None:
            self._labels_dev = self._images_dev.ctx.to_device(self.labels)
        return self._labels_dev

    def __len__(self):
        return len(self.sample_dirs)

    def __getitem__(self, idx):
        input_tensor = torch.from_numpy(np.ascontiguousarray(self.images[idx].transpose(2, 0, 1)))
        mask_tensor = torch.from_numpy(self.masks[idx].copy()).unsqueeze(0)
        if self.transform:
            input_tensor, mask_tensor = self.transform(input_tensor, mask_tensor)
        return input_tensor, mask_tensor
