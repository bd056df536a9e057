"""GPU: the HIP NLQ ensemble (`vilco_nlq_ensemble` via vilco_amd.utils.ensemble_nlq) against the imported reference's goldens
(tests/golden/nlq_ensemble.npz): every case bit-equal (`torch.equal` on fp64) from fp64 and, where the values allow, fp32
inputs; streams through `ensemble_streams` score like the reference's ensemble records; one launch per ensemble; the
single-list `temporal_nms` / `top1_generator`; identical output on consecutive launches."""
import json

import numpy as np
import pytest
import torch

import nlq_ensemble_restatement as R

pytestmark = pytest.mark.gpu
G = R.golden()
FP32_CASES = json.loads(str(G["fp32_cases"]))


def _device_case(name, dtype):
    from vilco_amd.utils import nlq_ensemble_device
    pred = torch.as_tensor(G[name + "__pred"]).to(dtype).cuda()
    cnt = torch.as_tensor(G[name + "__cnt"]).cuda()
    return nlq_ensemble_device(pred, cnt, want_proposals=True, **R.case_params(G, name))


@pytest.mark.parametrize("name,dtype", [(n, torch.float64) for n in R.case_names(G)] + [(n, torch.float32) for n in FP32_CASES])
def test_device_equals_reference_goldens(dev, name, dtype):
    out, out_cnt, prop, prop_cnt = _device_case(name, dtype)
    assert out.dtype == torch.float64 and out_cnt.dtype == torch.int32
    assert torch.equal(out.cpu(), torch.as_tensor(G[name + "__out"]))
    assert out.cpu().numpy().tobytes() == G[name + "__out"].tobytes()
    assert torch.equal(out_cnt.cpu(), torch.as_tensor(G[name + "__out_cnt"]))
    assert torch.equal(prop_cnt.cpu(), torch.as_tensor(G[name + "__prop_cnt"]))
    assert torch.equal(prop.cpu(), torch.as_tensor(G[name + "__prop"]))
    if name + "__mr" in G.files:
        assert torch.equal(out[:, :, :2].cpu(), torch.as_tensor(G[name + "__mr"]))
    again = _device_case(name, dtype)                                       # no atomics: the same bytes again
    for a, b in zip((out, out_cnt, prop, prop_cnt), again):
        assert torch.equal(a, b)


def test_query_counts_and_launches(dev):
    from vilco_amd.utils import ensemble_nlq as E
    pred = torch.as_tensor(G["bulk__pred"]).cuda()
    cnt = torch.as_tensor(G["bulk__cnt"]).cuda()
    before = E.LAUNCHES
    out, out_cnt = E.nlq_ensemble_device(pred[:, :0].contiguous(), cnt[:, :0].contiguous())
    assert E.LAUNCHES == before and tuple(out.shape) == (0, 5, 3) and tuple(out_cnt.shape) == (0,)     # no launch
    for n in (1, 5, 257):
        out, out_cnt = E.nlq_ensemble_device(pred[:, :n].contiguous(), cnt[:, :n].contiguous())
        assert torch.equal(out.cpu(), torch.as_tensor(G["bulk__out"][:n]))
        assert torch.equal(out_cnt.cpu(), torch.as_tensor(G["bulk__out_cnt"][:n]))
    assert E.LAUNCHES == before + 3


def _streams(ev, name, order=None):
    """the case's models as record streams (fp32 rows, as a model returns them)"""
    rows = R.case_rows(G, name)
    streams = []
    for m in range(len(rows[0])):
        st = ev.new_stream(capacity=4)
        for q in (order[m] if order else range(len(rows))):
            t = torch.tensor(rows[q][m], dtype=torch.float32, device="cuda")
            st.append(("c%d" % q, "a%d" % q, 0), t[:, :2], t[:, 2], seg_id=q % 3)
        streams.append(st)
    return streams


@pytest.mark.parametrize("name", ["bulk", "tail257"])
def test_streams_score_like_the_reference_records(dev, tmp_path, name):
    from vilco_amd.utils import NLQEnsembleStream, ensemble_nlq as E, ensemble_predictions, ensemble_streams, make_nlq_evaluator
    from nlq_metrics_restatement import write_ego4d
    ev = make_nlq_evaluator(write_ego4d(R.ego4d_gt(G[name + "__gt"]), tmp_path), dataset="ego4d")
    n = G[name + "__cnt"].shape[1]
    rng = np.random.default_rng(3)
    order = [list(range(n)), rng.permutation(n).tolist(), rng.permutation(n).tolist()]      # paired by key, not by position
    streams = _streams(ev, name, order)
    before = E.LAUNCHES
    ens = ensemble_streams(streams)
    assert E.LAUNCHES == before + 1 and isinstance(ens, NLQEnsembleStream) and len(ens) == n
    pred, cnt, gi, seg = ens.device_columns()
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (n, 5, 2) and pred.is_cuda
    assert torch.equal(pred.cpu(), torch.as_tensor(G[name + "__mr"]))
    assert torch.equal(ens.kept.cpu(), torch.as_tensor(G[name + "__out_cnt"]))
    # the reference's ensemble records
    ref = [{"query_idx": 0, "annotation_uid": "a%d" % q, "predicted_times": G[name + "__mr"][q].tolist(), "clip_uid": "c%d" % q}
           for q in range(n)]
    assert ens.records() == ref
    want, _ = ev.evaluate(ref, verbose=False)
    got, _ = ev.evaluate(ens, verbose=False)
    print(name, got.tolist())
    assert got.tobytes() == want.tobytes() and 0 < got[0, 0] <= got[0, 2] <= 1
    tables = ev.evaluate_segments(ens, verbose=False)
    assert len(tables) == 3 and tables[-1][0].tobytes() == want.tobytes()
    # record lists and files: every field of the first input's record, [start, end] rows
    lists = [[dict(r, extra=i) for i, r in enumerate(st.records())] for st in streams]
    path = str(tmp_path / "b.json")
    E.write_challenge_file(path, lists[1])
    before = E.LAUNCHES
    recs = ensemble_predictions([lists[0], path, lists[2]])
    assert E.LAUNCHES == before + 1
    assert recs == [dict(r, extra=i) for i, r in enumerate(ref)]
    assert len(lists[0][0]["predicted_times"]) == 5                                          # the inputs are left as they were
    # no padding: the counts travel with the stream
    nopad = ensemble_streams(streams, pad=False)
    assert [len(r["predicted_times"]) for r in nopad.records()] == G[name + "__out_cnt"].tolist()
    assert ev.evaluate(nopad, verbose=False)[0].tobytes() == want.tobytes()                  # the padding repeats a row


def test_command_line_writes_the_challenge_file(dev, tmp_path, capsys):
    from vilco_amd.utils import ensemble_nlq as E, make_nlq_evaluator
    from nlq_metrics_restatement import write_ego4d
    name = "m3"
    gt = write_ego4d(R.ego4d_gt(G[name + "__gt"] + [0.0, 4.0]), tmp_path)
    rows = R.case_rows(G, name)
    paths = []
    for m in range(3):
        paths.append(str(tmp_path / ("m%d.json" % m)))
        E.write_challenge_file(paths[-1], [{"query_idx": 0, "annotation_uid": "a%d" % q, "predicted_times": rows[q][m],
                                            "clip_uid": "c%d" % q} for q in range(len(rows))])
    out = str(tmp_path / "ens.json")
    assert E.main([out] + paths + ["--gt", gt]) == 0
    with open(out) as f:
        data = json.load(f)
    assert data["version"] == "1.0" and data["challenge"] == "ego4d_nlq_challenge"
    assert [r["predicted_times"] for r in data["results"]] == G[name + "__mr"].tolist()
    printed = capsys.readouterr().out
    want, table = make_nlq_evaluator(gt, dataset="ego4d").evaluate(data["results"], verbose=True)
    assert "Rank@1" in printed and table in printed
    assert E.main([out] + paths + ["--no-pad", "--nms-thd", "0.5"]) == 0
    with open(out) as f:
        assert [len(r["predicted_times"]) for r in json.load(f)["results"]] == G[name + "__out_cnt"].tolist()


def test_single_list_functions_equal_goldens(dev):
    from vilco_amd.utils import temporal_nms, top1_generator
    lst = G["tnms_in"].tolist()
    assert temporal_nms(lst, 0.5) == G["tnms_out"].tolist()                                  # max_after_nms = 100
    assert temporal_nms(torch.tensor(lst, dtype=torch.float32), 0.9, 7) == G["tnms_out_thd09_max7"].tolist()
    assert temporal_nms(G["tnms_one_in"].tolist(), 0.5) == G["tnms_one_out"].tolist()
    assert temporal_nms(lst, 0.5, max_after_nms=100) == R.temporal_nms(lst, 0.5)
    assert top1_generator(G["top1_in"].tolist()) == G["top1_out"].tolist()
    assert top1_generator(torch.tensor(G["top1_in"], dtype=torch.float32)) == G["top1_out"].tolist()
    for name in ("m2", "m3", "top2"):                                                        # the generator of the cases
        p = R.case_params(G, name)
        for q, models in enumerate(R.case_rows(G, name)):
            rows = [r for m in models for r in m[:p["top1_max_input"]]]
            want = G[name + "__prop"][q, :G[name + "__prop_cnt"][q]]
            assert top1_generator(rows) == [[s, e, w, 0, t] for s, e, w, t in want.tolist()]
    with pytest.raises(ValueError):
        temporal_nms([[0.0, 1.0, 0.5]] * 81, 0.5)
    with pytest.raises(ValueError):
        top1_generator([])
