"""GPU: engine.test_model (the reference's main.py:437-480, the --test_only entry) on the stub model and loader of
tests/test_gpu_engine_evaluate.py: a checkpoint in the reference's layout loads, --test_size prints the four blocks and returns the
host path's numbers, a missing checkpoint exits with status 1."""
from argparse import Namespace

import pytest
import torch

from test_gpu_engine_evaluate import DEV, _args, _fixture, _loader, _Stub

pytestmark = pytest.mark.gpu
SIZES = ("S", "M", "L")


def _checkpoint(path, model):
    """utils/io.py:23-29"""
    state = {k: torch.full_like(v, 5.0) for k, v in model.state_dict().items()}
    torch.save({"model": state, "optimizer": {"state": {}, "param_groups": []}, "epoch": 7,
                "args": Namespace(dataset_name="scannet", nqueries=256), "best_val_metrics": {}}, path)
    return str(path)


def test_checkpoint_loads_and_sizes_equal_the_host_path(tmp_path, capsys):
    from vdetr_amd import engine, eval_store
    from vdetr_amd.ap_calculator import APCalculator
    _, ds, outs, tgts = _fixture()
    model = _Stub(outs).to(DEV)
    args = _args(test_ckpt=_checkpoint(tmp_path / "checkpoint_best.pth", model), test_size=True)
    before = eval_store.MATCH_LAUNCHES
    ret = engine.test_model(args, model, model, "a criterion that must not be called", ds, {"test": _loader(tgts)})
    assert eval_store.MATCH_LAUNCHES - before == 2                         # the plain metrics, then S, M and L from one pass
    assert float(model.anchor.detach()) == 5.0 and model.anchor.device.type == "cuda" and model.calls == len(outs)
    text = capsys.readouterr().out
    want = APCalculator(dataset_config=ds, ap_iou_thresh=[0.25, 0.5], class2type_map=ds.class2type, no_nms=False, args=args)
    for out, tgt in zip(outs, tgts):
        want.step_meter({"outputs": {k: v.to(DEV) for k, v in out.items()}}, {k: v.to(DEV) for k, v in tgt.items()})
    assert list(ret) == ["", "S", "M", "L"]
    npos = sum(int((t["gt_box_present"] == 1).sum()) for t in tgts)
    blocks = text.split("=" * 20 + "\n")
    assert [b.split(";")[0] for b in blocks if b] == ["Evaluate ", "Test model", "Test model S", "Test model M", "Test model L"]
    for size in ret:
        host = want.compute_metrics(size)
        assert f"Test model{' ' + size if size else ''}; Metrics {want.metrics_to_str(host)}\n" in text
        for thr in (0.25, 0.5):
            assert list(ret[size][thr].keys()) == list(host[thr].keys())
            for key, w in host[thr].items():
                if key.endswith("Recall") or key == "AR":
                    assert float(ret[size][thr][key]) == float(w), (size, thr, key)
                else:   # two summation orders of at most npos + 1 terms; the float32 mAP may round the other way
                    assert abs(float(ret[size][thr][key]) - float(w)) <= (npos + 1) * 2.0 ** -52 + (2.0 ** -23 if key == "mAP" else 0), (size, thr, key)


def test_without_test_size_only_the_plain_metrics(tmp_path, capsys):
    from vdetr_amd import engine
    _, ds, outs, tgts = _fixture()
    model = _Stub(outs).to(DEV)
    args = _args(test_ckpt=_checkpoint(tmp_path / "c.pth", model), test_size=False)
    ret = engine.test_model(args, model, model, None, ds, {"test": _loader(tgts)})
    assert list(ret) == [""] and capsys.readouterr().out.count("Test model") == 1


@pytest.mark.parametrize("ckpt", [None, "no/such/checkpoint.pth"])
def test_missing_checkpoint_exits_with_status_1(ckpt):
    from vdetr_amd import engine
    _, ds, outs, tgts = _fixture()
    model = _Stub(outs).to(DEV)
    with pytest.raises(SystemExit) as e:
        engine.test_model(_args(test_ckpt=ckpt, test_size=True), model, model, None, ds, {"test": _loader(tgts)})
    assert e.value.code == 1 and model.calls == 0
