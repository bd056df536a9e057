"""CPU: the plain-Python restatement of the NLQ ensemble against the imported reference's goldens (tests/golden/nlq_ensemble.npz),
the required cases' presence in the fixture, the `vilco_nlq_ensemble` C-ABI entry (declared, in the table, exported; argument
checks without a device), pairing by key, and the challenge-file writer."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import nlq_ensemble_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.golden()


@pytest.mark.parametrize("name", R.case_names(G))
def test_restatement_matches_reference_goldens(name):
    out, out_cnt, prop, prop_cnt = R.ensemble_case(G, name)
    assert out.tobytes() == G[name + "__out"].tobytes()                      # bit-equal
    assert out_cnt.tolist() == G[name + "__out_cnt"].tolist()
    assert prop.tobytes() == G[name + "__prop"].tobytes() and prop_cnt.tolist() == G[name + "__prop_cnt"].tolist()
    if name + "__mr" in G.files:                                             # post_processing_mr_nms itself: [start, end]
        assert out[:, :, :2].tobytes() == G[name + "__mr"].tobytes()
        p = R.case_params(G, name)                                           # its constants: threshold 0.5, 5 rows, padded
        assert (p["nms_thd"], p["max_after_nms"], p["pad"], p["distance"]) == (0.5, 5, True, 2.0)


def test_restatement_single_lists():
    assert R.temporal_nms(G["tnms_in"].tolist(), 0.5) == G["tnms_out"].tolist()
    assert R.temporal_nms(G["tnms_in"].tolist(), 0.9, 7) == G["tnms_out_thd09_max7"].tolist()
    assert R.temporal_nms(G["tnms_one_in"].tolist(), 0.5) == G["tnms_one_out"].tolist()
    got = R.top1_generator(G["top1_in"].tolist())
    assert [[s, e, w, 0.0, t] for s, e, w, t in got] == G["top1_out"].tolist()


def test_fixture_holds_the_required_cases():
    names = R.case_names(G)
    fp32 = json.loads(str(G["fp32_cases"]))
    assert {G[n + "__cnt"].shape[0] for n in names} >= {1, 2, 3, 8}
    assert {G[n + "__cnt"].shape[1] for n in names} >= {1, 257, 300}
    assert "fp64" in names and "fp64" not in fp32 and len(fp32) == len(names) - 1
    par = {n: R.case_params(G, n) for n in names}
    assert {p["top1_max_input"] for p in par.values()} >= {0, 1, 2}
    assert {p["distance"] for p in par.values()} >= {1.0, 2.0, 4.0}
    assert {p["nms_thd"] for p in par.values()} >= {0.3, 0.5, 0.7}
    assert {p["pad"] for p in par.values()} == {True, False}
    assert par["m8"]["max_input"] == 10 and int(G["m8__cnt"].sum() + G["m8__prop_cnt"][0]) == 88
    kept = np.concatenate([G[n + "__out_cnt"] for n in names if par[n]["max_after_nms"] == 5])
    assert set(kept.tolist()) == {1, 2, 3, 4, 5}
    assert (G["m3__cnt"] == 1).any() and (G["m3__cnt"] == 5).any()          # one row; more rows than max_input
    pc, k = G["bulk__prop_cnt"], G["bulk__out_cnt"]
    assert min((pc == 1).sum(), (pc == 2).sum(), (pc == 3).sum(), (k < 5).sum()) >= 20
    assert len(G["tnms_out"]) > 5 and 0 < float(G["ref_seconds"]) < 60
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "nlq_ensemble.npz")) < 1 << 20


def test_abi_entry_declared_in_table_and_exported():
    from vilco_amd import _lib
    with open(os.path.join(ROOT, "include", "vilco_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint vilco_nlq_ensemble\(([^;]*)\);", header)
    assert m and "vilco_nlq_ensemble" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["vilco_nlq_ensemble"]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == 17
    assert args[8] is ctypes.c_double and args[9] is ctypes.c_double and args[4] is ctypes.c_int64
    assert hasattr(_lib.load(), "vilco_nlq_ensemble")
    with open(os.path.join(ROOT, "vilco_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert mk.count("ensemble.o") == 2 and "ensemble.hip" in mk              # both -ffp-contract=off rules


def test_abi_rejects_bad_arguments_without_a_device():
    from vilco_amd import _lib
    lib = _lib.load()
    d = 256

    def call(pred=d, fp32=0, cnt=d, n_model=3, n=100, k_cap=5, max_input=4, top1=1, distance=2.0, thd=0.5, max_after=5, pad=1,
             out=d, out_cnt=d, prop=None, prop_cnt=None):
        return lib.vilco_nlq_ensemble(pred, fp32, cnt, n_model, n, k_cap, max_input, top1, distance, thd, max_after, pad, out,
                                      out_cnt, prop, prop_cnt, None)
    for kw in (dict(pred=None), dict(cnt=None), dict(out=None), dict(out_cnt=None), dict(n=-1), dict(n_model=0),
               dict(n_model=9), dict(max_input=0), dict(max_input=-1), dict(max_input=11, k_cap=11), dict(k_cap=3),
               dict(top1=-1), dict(max_after=0), dict(max_after=-5), dict(max_after=129), dict(n_model=8, top1=9, k_cap=9),
               dict(n_model=8, max_input=10, k_cap=10, top1=7), dict(prop=d), dict(prop_cnt=d), dict(pred=d + 4),
               dict(pred=d + 2, fp32=1), dict(out=d + 4), dict(prop=d + 4, prop_cnt=d)):
        assert call(**kw) == -1, kw
    # no queries: nothing to do, null pointers allowed
    assert call(pred=None, cnt=None, out=None, out_cnt=None, n=0) == 0
    assert call(pred=None, cnt=None, out=None, out_cnt=None, n=0, max_input=0) == -1


def _recs(n, shift=0.0, keys=None):
    return [{"query_idx": 0, "annotation_uid": "a%d" % q, "clip_uid": "c%d" % q, "extra": q,
             "predicted_times": [[1.0 + shift, 5.0 + shift, 0.5]]} for q in (keys if keys is not None else range(n))]


def test_key_mismatch_raises():
    import torch
    from vilco_amd.utils import ensemble_predictions, ensemble_streams, ensemble_nlq as E
    from vilco_amd.utils.metrics_nlq import NLQRecordStream
    with pytest.raises(ValueError, match="different queries"):
        ensemble_predictions([_recs(4), _recs(0, keys=[0, 1, 2, 7])])
    with pytest.raises(ValueError, match="different queries"):
        ensemble_predictions([_recs(4), _recs(3)])
    with pytest.raises(ValueError, match="twice"):
        ensemble_predictions([_recs(3), _recs(0, keys=[0, 1, 1, 2])])
    with pytest.raises(ValueError, match="at least one row"):
        ensemble_predictions([_recs(2), [dict(r, predicted_times=[]) for r in _recs(2)]])
    with pytest.raises(ValueError):
        ensemble_predictions([_recs(2)] * 9)
    with pytest.raises(TypeError):
        ensemble_predictions([_recs(2)], max_inputs=3)
    assert E._pair([["a", "b", "c"], ["c", "a", "b"]]) == [[0, 1, 2], [1, 2, 0]]
    streams = []
    for keys in (("x", "y"), ("x", "z")):
        st = NLQRecordStream(lambda key: 0, k_cap=5, capacity=2, device="cpu")
        for k in keys:
            st.append(("c", k, 0), torch.tensor([[1.0, 2.0]]), torch.tensor([0.5]))
        streams.append(st)
    with pytest.raises(ValueError, match="different queries"):
        ensemble_streams(streams)


def test_challenge_file_round_trips(tmp_path):
    from vilco_amd.utils import ensemble_nlq as E
    recs = _recs(5)
    path = str(tmp_path / "ens.json")
    E.write_challenge_file(path, recs)
    with open(path) as f:
        data = json.load(f)
    assert sorted(data) == ["challenge", "results", "version"]
    assert data["version"] == "1.0" and data["challenge"] == "ego4d_nlq_challenge"
    assert E.load_predictions(path) == recs
    bare = str(tmp_path / "bare.json")
    with open(bare, "w") as f:
        json.dump(recs, f)
    assert E.load_predictions(bare) == recs
