#!/usr/bin/env python3
"""Golden fixtures for the random-input checks of the NMS and ROIAlign oracles, recorded from the REFERENCE'S OWN CPU KERNELS.

    python oracle/build_ref.py && python tests/golden/make_golden_ref_live.py

tests/test_oracle_nms.py::test_oracle_edge_cases_and_live_binary and
tests/test_oracle_roi.py::test_oracle_matches_reference_binary_live_when_present hold the oracles to the compiled reference kernels
(oracle/_ref/) on seeded random inputs.  That module can only be built where the reference sources are; this file stores the
same inputs and the reference's outputs for them, so the tests check the oracles bit for bit wherever they run, and additionally
against the live module when it is present.

  nms_<n>_*  : torch.Generator seed 3, (n, threshold) in NMS_CASES -- dets [n,4], scores [n], the kept indices
  roi_*      : torch.Generator seed 7, an image [3,2,61,83], 40 rois (partly outside, some malformed), the output of every
               (pooled h, pooled w, sampling_ratio, spatial_scale) in ROI_SETTINGS
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from oracle import build_ref  # noqa: E402

PATH = os.path.join(HERE, "ref_live_golden.npz")
NMS_CASES = [(300, 0.6), (77, 0.2)]
ROI_SETTINGS = [(7, 7, 0, 1.0), (5, 9, 2, 0.5), (16, 16, 0, 1.0)]


def nms_inputs():
    """-> [(n, thr, dets [n,4], scores [n])] in NMS_CASES order (one generator across the cases)."""
    g = torch.Generator().manual_seed(3)
    out = []
    for n, thr in NMS_CASES:
        xy = torch.rand(n, 2, generator=g) * 200
        wh = torch.rand(n, 2, generator=g) * 80 + 1
        out.append((n, thr, torch.cat([xy, xy + wh], 1), torch.rand(n, generator=g)))
    return out


def roi_inputs():
    """-> image [3,2,61,83], rois [40,5] (batch index, x1, y1, x2, y2)."""
    g = torch.Generator().manual_seed(7)
    img = torch.rand(3, 2, 61, 83, generator=g)
    xy = torch.rand(40, 2, generator=g) * torch.tensor([90.0, 70.0]) - 5
    wh = torch.rand(40, 2, generator=g) * torch.tensor([70.0, 60.0]) - 2
    rois = torch.cat([torch.randint(0, 3, (40, 1), generator=g).float(), xy, xy + wh], 1)
    return img, rois


def load():
    return np.load(PATH, allow_pickle=False)


def main():
    ref = build_ref.load() or (build_ref.build() and build_ref.load())
    assert ref is not None, "run oracle/build_ref.py first (needs the reference sources)"
    out = {}
    for n, thr, dets, scores in nms_inputs():
        out[f"nms_{n}_dets"], out[f"nms_{n}_scores"] = dets.numpy(), scores.numpy()
        out[f"nms_{n}_thr"] = np.array(thr)
        out[f"nms_{n}_keep"] = ref.nms(dets, scores, thr).numpy().astype(np.int64)
        print("nms", n, thr, "kept", len(out[f"nms_{n}_keep"]))
    img, rois = roi_inputs()
    out["roi_img"], out["roi_rois"] = img.numpy(), rois.numpy()
    for k, (ph, pw, sr, scale) in enumerate(ROI_SETTINGS):
        out[f"roi_out{k}"] = ref.roi_align_forward(img, rois, scale, ph, pw, sr).numpy()
        print("roi", (ph, pw, sr, scale), out[f"roi_out{k}"].shape)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH))


if __name__ == "__main__":
    main()
