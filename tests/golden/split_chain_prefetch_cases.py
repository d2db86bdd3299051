"""Cases of tests/test_gpu_split_chain_prefetch.py, shared with the recorder of its fixtures (tools/record_split_chain_prefetch.py):
the two production recurrent builds (exact split, two workgroups per CU) at the smallest shapes where the fragment schedule of
split_chain (csrc/coop_common.h) can go wrong.  B = 17: two tiles, the second with one live row and a tile switch.

Encoder, L in ENC_LENGTHS: 1 = no product; 2 = the first product, on a cold prefetch; 3 = both step parities; 9 = the k-block
double buffers wrap around several times per step, over several steps.  Decoder, (T, K) in DEC_SHAPES: one, two and three decoded
steps, K = 5 and K = 10 (one and two lanes per partial dot: both production decoder builds); Low and High in one launch."""
import numpy as np
import torch

from oracle import pn as opn

H, B = 256, 17
ENC_LENGTHS = (1, 2, 3, 9)
DEC_SHAPES = ((1, 5), (2, 5), (3, 10))
SEED_LOW, SEED_HIGH = 731, 732
KEPT_ROWS = (0, 15, 16)          # decoder cases keep enc_out of these problems in full (first and last row of tile 0, the one row of tile 1)
FIXTURE_DIR = "split_chain_prefetch"   # under tests/golden: recorded on the GPU from a library, not written by the generators of MANIFEST.json
ENC_FIXTURE, DEC_FIXTURE = FIXTURE_DIR + "/enc.npz", FIXTURE_DIR + "/dec.npz"


def make_inputs(L, K):
    g = torch.Generator().manual_seed(1000 * L + K)
    x = torch.rand(B, L, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    return x


def build_nets(T, K, dev):
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    nets = []
    for level, seed in (("Low", SEED_LOW), ("High", SEED_HIGH)):
        m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, seed), strict=True)
        nets.append(m.to(dev).eval())
    return nets


def _drop_packed_split(nets):
    for m in nets:                       # the same weights without the packed image: the kernels split for themselves
        m.actor.packed().pop("enc_whh_split")
        m.actor.packed().pop("dec_whh_split")


def bit_sums(t):
    """Sum of the bit patterns of every problem's rows, [..., B] int64: any changed bit of a tensor too large to keep changes it."""
    return t.contiguous().view(torch.int32).to(torch.int64).flatten(2).sum(-1)


def run_encoder(dev, L, x, write_through, packed):
    """Both nets' encoder recurrences in one launch -> {enc_out [2,B,L,H], h_n, c_n [2,B,H]} (numpy)."""
    from gnnpn_sc_amd import ops
    low, high = build_nets(1, L, dev)
    if not packed:
        _drop_packed_split((low, high))
    args = [m.actor.encode_args(x.to(dev))[0] for m in (low, high)]
    assert all((a.get("whh_split") is not None) == packed for a in args)
    enc, h_n, c_n = ops.lstm_encode(args, precision="split", write_through=write_through)
    ops.check_status(dev)
    return {k: torch.stack(v).cpu().numpy() for k, v in (("enc_out", enc), ("h_n", h_n), ("c_n", c_n))}


def run_decoder(dev, T, K, x, write_through, packed):
    """Encoders, then Low and High decoded in one launch of the two-per-CU exact-split build (decode_impl 4)."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import _two_level_fused
    low, high = build_nets(T, K, dev)
    if not packed:
        _drop_packed_split((low, high))
    xd = x.to(dev)
    args = [m.actor.encode_args(xd)[0] for m in (low, high)]
    enc, h_n, c_n = ops.lstm_encode(args, precision="split", write_through=write_through)
    out = _two_level_fused(low, high, xd, None, "split", 4, 0, write_through, None, None, False)[0]
    ops.check_status(dev)
    enc = torch.stack(enc)
    res = {"enc_rows": enc[:, list(KEPT_ROWS)].cpu().numpy(), "enc_bits": bit_sums(enc).cpu().numpy(),
           "h_n": torch.stack(h_n).cpu().numpy(), "c_n": torch.stack(c_n).cpu().numpy()}
    for k in ("idx_low", "idx_high", "win_low", "win_high_raw", "R", "actions", "action_probs"):
        res[k] = out[k].cpu().numpy()
    return res


def enc_key(L, name):
    return f"L{L}_{name}"


def dec_key(T, K, name):
    return f"T{T}K{K}_{name}"


def record(dev):
    """-> (encoder fixture, decoder fixture) as dicts of arrays: the packed-weights, same-XCD hand-off run of every case."""
    enc, dec = {}, {}
    for L in ENC_LENGTHS:
        x = make_inputs(L, 0)
        enc[enc_key(L, "x")] = x.numpy()
        r = run_encoder(dev, L, x, False, True)
        assert np.array_equal(r["h_n"], r["enc_out"][:, :, L - 1])      # (h_n is the last row of enc_out: not stored)
        enc[enc_key(L, "enc_out")], enc[enc_key(L, "c_n")] = r["enc_out"], r["c_n"]
    for T, K in DEC_SHAPES:
        x = make_inputs(T * K, K)
        dec[dec_key(T, K, "x")] = x.numpy()
        for k, v in run_decoder(dev, T, K, x, False, True).items():
            dec[dec_key(T, K, k)] = v
    return enc, dec
