"""The reference NMS extension's own outputs (oracle/_ref/nms_1d_cpu.so, built from the reference's nms_cpu.cpp by
oracle/build_ref.py) on the cases of tests/test_oracle_nms.py::test_against_reference_build, so that the test pins the
numpy restatement to the reference build on machines without it.
Run:  python tests/golden/make_golden_nms_ref.py  ->  tests/golden/nms_ref_build.pt"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import build_ref  # noqa: E402
from test_oracle_nms import REF_CASES, REF_SOFT, make_case  # noqa: E402


def main():
    ref = build_ref.load_ref()
    assert ref is not None, "reference extension not built"
    rec = {}
    for n, ties in REF_CASES:
        segs, scores = make_case(n, 11 + n, ties)
        ts, tc = torch.from_numpy(segs).reshape(-1, 2), torch.from_numpy(scores)
        soft = []
        for sigma, ms in REF_SOFT:
            dets = torch.zeros(n, 3)
            inds = ref.softnms(ts, tc, dets, 0.1, sigma, ms, 2)
            soft.append((inds.numpy(), dets.numpy()[:len(inds)].copy()))
        rec["%d_%d" % (n, ties)] = {"hard": None if ties else ref.nms(ts, tc, 0.4).numpy(), "soft": soft}
    torch.save(rec, os.path.join(HERE, "nms_ref_build.pt"))


if __name__ == "__main__":
    main()
