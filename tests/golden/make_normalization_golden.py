#!/usr/bin/env python3
"""Write the normalisation fixtures with the REFERENCE's own code and scikit-learn 1.7.2.

Run in the build container only (the reference never travels), with the reference checkout on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_normalization_golden.py

Under ``np.random.seed`` four reference ``RFISimulator(time_bins=64, freq_bins=64).generate_rfi()`` samples are
written with the reference's ``save_example_pair_npy`` into a temporary directory.  Recorded:

  normalization_inputs.npz              the four (8, 64, 64) fp64 inputs and masks in the order of the reference
                                        dataset's ``sample_dirs`` (``os.listdir`` order) with their directory names;
                                        a constant sample (0.5 everywhere, so every sum is exact); a two-valued
                                        sample whose 25 % and 75 % quantiles coincide
  normalization_expected.npz            the reference ``RFIMaskDataset``'s attributes for the three methods, over the
                                        four samples and over each degenerate sample alone (with its items)
  normalization_expected_dataset_<m>.npz   ``RFIMaskDataset.__getitem__`` float32 outputs of every sample, method m
  normalization_expected_sample_<m>.npz    ``normalize_array`` outputs of all six samples, cast to float32 as
                                        ``torch.tensor(..., dtype=torch.float32)`` casts them, method m

(one file per method: a committed file stays below 1 MiB).  The files are DATA produced by reference code; nothing of
its source is stored.
"""
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ("global_min_max", "standardize", "robust_scale")
ATTRS = ("global_min", "global_max", "mean", "std", "robust_median", "robust_iqr")


def dataset_record(RFIMaskDataset, root, prefix, out, items_out=None):
    for m in METHODS:
        ds = RFIMaskDataset(root, normalization=m)
        for a in ATTRS:
            v = getattr(ds, a)
            out[f"{prefix}{m}.{a}"] = np.float64(np.nan if v is None else v)
        out[f"{prefix}{m}.has_robust"] = np.bool_(ds.robust_median is not None)
        items = np.stack([ds[i][0].numpy() for i in range(len(ds))])
        masks = np.stack([ds[i][1].numpy() for i in range(len(ds))])
        assert items.dtype == np.float32 and masks.dtype == np.float32
        if items_out is None:
            out[f"{prefix}{m}.items"] = items
        else:
            items_out[m] = (items, masks)
    return ds.sample_dirs


def main():
    import sklearn
    from rfi_toolbox.core.simulator import RFISimulator
    from rfi_toolbox.datasets.rfi_mask_dataset import RFIMaskDataset
    from rfi_toolbox.scripts.generate_dataset import save_example_pair_npy
    from rfi_toolbox.scripts.normalize_rfi_data import normalize_array

    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    np.random.seed(20251017)
    sim = RFISimulator(time_bins=64, freq_bins=64)
    expected, items = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "four")
        for i in range(4):
            tf_plane, mask = sim.generate_rfi()
            save_example_pair_npy(tf_plane, mask, i, root)
        dirs = dataset_record(RFIMaskDataset, root, "four.", expected, items)
        names = [os.path.basename(d) for d in dirs]
        inputs = np.stack([np.load(os.path.join(d, "input.npy")) for d in dirs])
        masks = np.stack([np.load(os.path.join(d, "rfi_mask.npy")) for d in dirs])
        assert inputs.shape == (4, 8, 64, 64) and inputs.dtype == np.float64

        constant = np.full((8, 64, 64), 0.5)
        rng = np.random.RandomState(7)
        two_valued = np.where(rng.rand(8, 64, 64) < 0.8, 1.0, 3.0)
        assert np.percentile(two_valued, 25) == np.percentile(two_valued, 75) == 1.0
        for name, x in (("constant", constant), ("two_valued", two_valued)):
            d = os.path.join(tmp, name, "0000")
            os.makedirs(d)
            np.save(os.path.join(d, "input.npy"), x)
            np.save(os.path.join(d, "rfi_mask.npy"), np.zeros((64, 64), dtype=bool))
            dataset_record(RFIMaskDataset, os.path.join(tmp, name), name + ".", expected)

    np.savez_compressed(os.path.join(HERE, "normalization_inputs.npz"), inputs=inputs, masks=masks, names=np.array(names),
                        constant=constant, two_valued=two_valued)
    np.savez_compressed(os.path.join(HERE, "normalization_expected.npz"), **expected)
    six = list(inputs) + [constant, two_valued]
    for m in METHODS:
        np.savez_compressed(os.path.join(HERE, f"normalization_expected_dataset_{m}.npz"), items=items[m][0], masks=items[m][1])
        per_sample = np.stack([np.asarray(normalize_array(x.copy(), method=m)).astype(np.float32) for x in six])
        np.savez_compressed(os.path.join(HERE, f"normalization_expected_sample_{m}.npz"), outputs=per_sample)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("normalization_"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
