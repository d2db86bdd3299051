"""-m gpu: ML2PNPipeline.run with the one-launch score product + candidate reduction against the same pipeline with
GNNPN_UNFUSED_FRONT=1 (linear + segment_topk_feasible), eagerly and through ``capture``: every key of the output dict equal
(torch.equal).  B = 33 (two full tiles of 16 problems and a tile of one), T = 6, 20 services per category."""
import pytest
import torch

from conftest import eager_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(dev):
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd.modelML import Net
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices, ML2PNPipeline
    from oracle import ml as oml, pn as opn
    T, S, K, B, H = 6, 120, 3, 33, 256
    table = synth.make_service_table(T, S, seed=11, degree=8)
    pb = synth.make_problem_batch(table, B, seed=12, tasks_per_problem=4, lo_range=(0.85, 0.96))
    net = Net(128, S, 20, 2, 2)
    net.load_state_dict(oml.make_state_dict(128, 20, 2, 2, seed=13))
    low = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level="Low")
    high = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level="High")
    low.load_state_dict(opn.make_state_dict(H, 8))
    high.load_state_dict(opn.make_state_dict(H, 9))
    pipe = ML2PNPipeline(net.to(dev).eval(), low.to(dev).eval(), high.to(dev).eval(), K)
    return pipe, DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_run_fused_equals_unfused_eager_and_captured(setup, monkeypatch):
    from gnnpn_sc_amd import ops
    pipe, svc, batch = setup
    monkeypatch.setenv("GNNPN_UNFUSED_FRONT", "1")
    assert pipe.score_select_operands(svc, batch) is None
    want = {k: v.clone() for k, v in eager_reference(pipe, svc, batch).items()}
    replay = pipe.capture(svc, batch)
    want_graph = {k: v.clone() for k, v in replay().items()}
    ops.check_status(batch.x.device)
    _same(want_graph, want)
    monkeypatch.delenv("GNNPN_UNFUSED_FRONT")
    assert pipe.score_select_operands(svc, batch) is not None          # 20 services per category, hidden 128: the fused kernel applies
    got = eager_reference(pipe, svc, batch)
    _same(got, want)
    replay = pipe.capture(svc, batch)
    got_graph = replay()
    ops.check_status(batch.x.device)
    _same(got_graph, want)
