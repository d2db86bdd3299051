"""-m gpu: every cooperative kernel decodes the launch-flag word (csrc/coop_common.h: COOP_FLAG_*) the same way.

Results cannot see a swapped or ignored write-through bit — both hand-off forms give the same bits — but the launch's own status
area can: a seated workgroup that hands off inside its XCD counts itself into COOP_PLACED_OFFSET, one that writes through does not.
Shape: hidden 256, n_cat = n_per = 2, B = 17 — two tiles, the second with one live row (the smallest shape with a tile switch).
There the launch protocol gives one group per XCD, i.e. 8 groups of 8 members, every group with a net, for one net and for two:
64 workgroups counted by default, none with write_through.  (Paired start has no deterministic observable at this size: the
pipeline tests cover it.)"""
import pytest
import torch

from test_gpu_pn import build

pytestmark = pytest.mark.gpu

CFG = {"hidden": 256, "n_cat": 2, "n_per": 2, "seed_low": 31, "seed_high": 32}
B = 17
SEATED = 64      # 8 XCDs x 1 group x 8 members


def _encoder(precision):
    def run(low, high, x, ws, write_through):
        from gnnpn_sc_amd import ops
        nets = [m.actor.encode_args(x, None)[0] for m in (low, high)]
        enc, h_n, c_n = ops.lstm_encode(nets, precision=precision, ws=ws, write_through=write_through)
        return dict(enumerate(enc + h_n + c_n)), ws._encode
    return run


def _decoder(**kw):
    def run(low, high, x, ws, write_through):
        from gnnpn_sc_amd.modelPN import two_level_greedy
        return two_level_greedy(low, high, x, decode_impl=2, ws=ws, write_through=write_through, **kw), ws._decode
    return run


LAUNCHES = {
    "encoder_f32": _encoder("f32"),
    "encoder_split": _encoder("split"),
    "lean_f32": _decoder(precision="f32"),                                   # pointer_decode_lean_kernel<false, ...>
    "lean_split": _decoder(precision="split"),                               # pointer_decode_lean_kernel<true, ...>
    "coop_unfolded": _decoder(precision="f32", fold=False),                  # pointer_decode_coop_kernel<false, false>
    "coop_sampled": _decoder(precision="f32", sample_high_seed=7),           # pointer_decode_coop_kernel<true, true>
}


@pytest.fixture(scope="module")
def nets_and_inputs(dev):
    low, high = build(CFG, dev)
    x = torch.rand(B, CFG["n_cat"] * CFG["n_per"], 8, generator=torch.Generator().manual_seed(3))
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    return low, high, x.to(dev)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_write_through_flag_reaches_the_kernel(dev, nets_and_inputs, name):
    from gnnpn_sc_amd import ops
    low, high, x = nets_and_inputs
    placed, outs = {}, {}
    for write_through in (False, True):
        ws = ops.new_workspaces(dev)
        outs[write_through], area = LAUNCHES[name](low, high, x, ws, write_through)
        ws.check()                                                           # synchronises; clean
        words = area[:ops.COOP_STATUS_BYTES].view(torch.int32)
        placed[write_through] = int(ops.coop_per_xcd(words, ops.COOP_PLACED_OFFSET).sum().item())
    print(f"{name}: workgroups on the same-XCD hand-off: default {placed[False]}, write_through {placed[True]}")
    assert outs[False].keys() == outs[True].keys()
    for key in outs[False]:
        assert torch.equal(outs[False][key], outs[True][key]), key
    assert placed[False] == SEATED
    assert placed[True] == 0
