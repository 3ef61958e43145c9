"""Generate tests/golden/ground_truth.npz (data only, compressed) from the reference's bundled explanation files.

Run in the build container (reads /root/reference):  python tests/golden/make_ground_truth_golden.py

  gt_all               explanation_datasets/gt_all.csv (1754 x 378: obj, rel, sbj, then up to 125 ground-truth
                       triples flattened) as int32, the CSV's empty cells as -1
  test_filtered_fold4  explanation_datasets/test_filtered_fold4.csv (288 x 3), gt_process.py's output
  fold4_X_test         prediction_datasets/mode0_fold4_X_test.csv (700 x 3), gt_process.py's input
The pickled gt_filtered_fold4.npz is not loaded (no unpickling of reference files): the tests re-derive it.
"""
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
DS = "/root/reference/datasets"


def main():
    gt = pd.read_csv(f"{DS}/explanation_datasets/gt_all.csv").to_numpy(dtype=np.float64)
    assert np.all(np.isnan(gt) | (gt == np.round(gt))) and np.nanmax(gt) < 2 ** 31 and np.nanmin(gt) >= 0
    gt_all = np.where(np.isnan(gt), -1, gt).astype(np.int32)
    test = pd.read_csv(f"{DS}/explanation_datasets/test_filtered_fold4.csv").to_numpy().astype(np.int32)
    x_test = pd.read_csv(f"{DS}/prediction_datasets/mode0_fold4_X_test.csv").to_numpy().astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "ground_truth.npz"), gt_all=gt_all, test_filtered_fold4=test,
                        fold4_X_test=x_test)
    print(gt_all.shape, test.shape, x_test.shape)


if __name__ == "__main__":
    main()
