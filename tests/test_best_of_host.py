"""-m "not gpu": best-of-N decoding without a GPU — the new entry points (gnnpn_pointer_decode_replicas_f32,
gnnpn_best_of_select_f32) reject bad arguments before any launch, replica_seed agrees with the header's definition, the
selection rule restated in numpy, and `main.py ... --samples=N` parsing."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced
M64 = 0xFFFFFFFFFFFFFFFF


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib, _lib.load()


def _header_replica_seed(seed, i):
    """include/gnnpn_hip.h: replica_seed(seed, i) = fmix(seed ^ (i * 0xD1B54A32D192ED03)) & (2^63 - 1), in numpy uint64
    arithmetic."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) ^ (np.uint64(i & M64) * np.uint64(0xD1B54A32D192ED03))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int((z ^ (z >> np.uint64(31))) & np.uint64(0x7FFFFFFFFFFFFFFF))


FIXED = [(0, 0, 0x0), (1, 1, 0x1d60447fea35413), (7, 3, 0x4f6f752e6ed16e74), (2**63 + 5, 31, 0x083c606003a3e11c)]


def test_replica_seed_matches_the_header_definition():
    from gnnpn_sc_amd import ops
    _, lib = _lib()
    for s, j, want in FIXED:
        assert _header_replica_seed(s, j) == want
        assert ops.replica_seed(s, j) == want
        assert lib.gnnpn_replica_seed(s, j) == want
    for s in (0, 5, 123456789, 2**64 - 1):
        for j in range(40):
            assert ops.replica_seed(s, j) == lib.gnnpn_replica_seed(s, j) == _header_replica_seed(s, j)
    # a hash, not an offset: no replica's seed is another's plus a multiple of the stream's golden step
    golden = 0x9E3779B97F4A7C15
    seeds = [ops.replica_seed(11, j) for j in range(1, 33)]
    assert len(set(seeds)) == 32 and all(0 <= s < 2**63 for s in seeds)     # the range custom_ops passes on
    assert all((b - a) & M64 not in (golden, (-golden) & M64) for a in seeds for b in seeds)


def _decode_net(lib_mod, **over):
    d = lib_mod.DecodeNet()
    for n in ("enc_out", "h0", "c0", "start", "wih_packed", "whh_packed", "bih", "bhh", "latent_win", "xw_fold", "xb_fold",
              "start_fold", "idx", "win_logits", "pick_prob", "actions"):
        setattr(d, n, 64)
    d.latent_from = -1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_replica_decode_rejects_bad_arguments():
    lib_mod, lib = _lib()
    opts = lib_mod.LaunchOpts()

    def call(net=None, inputs=P, B=256, R=15, first=1, T=47, K=5, H=256, ws=P, ws_bytes=1 << 40, opt=opts):
        net = _decode_net(lib_mod) if net is None else net
        return lib.gnnpn_pointer_decode_replicas_f32(ctypes.byref(net), inputs, 10.0, 1, B, R, first, 7, T, K, H,
                                                     ctypes.byref(opt), ws, ws_bytes, None)
    for kw, msg in (({"R": 0}, b"R must be"), ({"R": -3}, b"R must be"), ({"first": -1}, b"first replica"),
                    ({"B": -1}, b"bad shape"), ({"T": 0}, b"bad shape"), ({"K": 0}, b"bad shape"), ({"K": 65}, b"bad shape"),
                    ({"B": 1 << 20, "R": 1 << 12}, b"exceed"), ({"inputs": None}, b"null input")):
        assert call(**kw) == -1, kw
        assert msg in lib.gnnpn_last_error(), (kw, lib.gnnpn_last_error())
    assert call(H=64) == -2                                          # hidden size not built
    for field in ("enc_out", "h0", "c0", "whh_packed"):
        assert call(net=_decode_net(lib_mod, **{field: None})) == -1 and b"null input" in lib.gnnpn_last_error()
    for field in ("idx", "actions", "pick_prob", "win_logits"):
        assert call(net=_decode_net(lib_mod, **{field: None})) == -1 and b"null output" in lib.gnnpn_last_error()
    assert call(net=_decode_net(lib_mod, xb_fold=None)) == -1 and b"go together" in lib.gnnpn_last_error()
    assert call(net=_decode_net(lib_mod, queries=64)) == -1 and b"queries" in lib.gnnpn_last_error()
    assert call(net=_decode_net(lib_mod, latent_from=0)) == -1 and b"latent_from" in lib.gnnpn_last_error()
    bad = lib_mod.LaunchOpts()
    bad.impl = 4
    assert call(opt=bad) == -1 and b"impl" in lib.gnnpn_last_error()
    # B*R rows beyond the workspace: refused before the launch (the size needed grows with the rows)
    assert call(ws_bytes=4096) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert call(ws=None, ws_bytes=0, opt=_impl(lib_mod, 2)) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert b"3840 rows" in (call(ws_bytes=4096), lib.gnnpn_last_error())[1]
    # the streaming form needs the embedded tensor
    assert call(opt=_impl(lib_mod, 1)) == -2 and b"embedded" in lib.gnnpn_last_error()
    assert call(B=0, inputs=None) == 0                               # an empty batch launches nothing


def _impl(lib_mod, impl):
    o = lib_mod.LaunchOpts()
    o.impl = impl
    return o


def test_best_of_select_rejects_bad_arguments():
    _, lib = _lib()

    def call(B=4, N=3, T=5, R0=P, Rs=P, idxs=P, winner=P):
        return lib.gnnpn_best_of_select_f32(B, N, T, R0, P, P, P, Rs, idxs, P, P, P, P, P, P, winner, None)
    for kw in ({"B": -1}, {"N": 0}, {"T": 0}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert call(R0=None) == -1 and b"replica 0" in lib.gnnpn_last_error()
    assert call(Rs=None) == -1 and b"replicas 1..N-1" in lib.gnnpn_last_error()
    assert call(idxs=None) == -1 and b"replicas 1..N-1" in lib.gnnpn_last_error()
    assert call(winner=None) == -1 and b"null output" in lib.gnnpn_last_error()
    assert call(B=0, R0=None, Rs=None) == 0


def test_replica_wrappers_refuse_host_tensors():
    import torch
    from gnnpn_sc_amd import ops
    g = {"R": torch.zeros(2), "idx": torch.zeros((2, 3), dtype=torch.int32), "actions": torch.zeros((2, 3, 8)),
         "probs": torch.zeros((2, 3))}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.best_of_select(g)


def select_rule(R_all):
    """The selection restated: per problem the replica with the smallest R, the lowest index among equal R (greedy, replica 0,
    wins every tie); NaN never wins against a number."""
    R = np.where(np.isnan(R_all), np.inf, R_all)
    return np.argmin(R, axis=1)


def test_selection_rule_with_ties():
    R_all = np.array([[0.5, 0.5, 0.4, 0.4],        # tie between 2 and 3 -> 2
                      [0.3, 0.3, 0.3, 0.3],        # all equal -> greedy
                      [1.2, 0.9, np.nan, 0.9],     # NaN skipped, tie -> 1
                      [np.nan, np.nan, 2.0, 1.0],  # greedy NaN -> 3
                      [0.0, -0.0, 0.1, 0.2]],      # -0 == +0 -> greedy
                     dtype=np.float32)
    assert select_rule(R_all).tolist() == [2, 0, 1, 3, 0]
    rng = np.random.default_rng(5)
    for _ in range(200):                           # 5-decimal rewards: ties are common
        R = np.round(rng.integers(0, 3, size=(16, 8)) + rng.integers(0, 4, size=(16, 8)) / 4, 5).astype(np.float32)
        w = select_rule(R)
        best = R.min(1)
        assert np.array_equal(R[np.arange(16), w], best) and (best <= R[:, 0]).all()
        assert all(w[b] == int(np.flatnonzero(R[b] == best[b])[0]) for b in range(16))


def test_main_parses_samples_and_keeps_the_epoch(monkeypatch, tmp_path):
    """`main.py QWS ML+2PN 3 --infer --random-init --samples=4 --seed 7`: samples=4, sample_seed=7, epoch 3; without
    --samples, infer gets no new keyword at all."""
    import json
    import main as cli
    from gnnpn_sc_amd import ML2PN
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "QWS").mkdir(parents=True)
    (tmp_path / "data" / "QWS" / "serviceFeature.data").write_text(json.dumps({"1": [[0.1] * 4] * 3, "2": [[0.2] * 4] * 2}))
    (tmp_path / "environment.ini").write_text("[QWS-ML+2PN]\nserviceCategory = 2\nepoch = -1\n")
    seen = []
    monkeypatch.setattr(cli, "_models", lambda cfg, ds, n_services, n_cat, epoch, random_init: ("net", "low", "high", 3))
    monkeypatch.setattr(ML2PN, "infer", lambda *a, **k: seen.append((a, k)))
    monkeypatch.setattr(ML2PN, "check", lambda ds, n_cat, epoch: seen.append(("check", epoch)))
    assert cli.main(["main.py", "QWS", "ML+2PN", "3", "--infer", "--random-init", "--samples=4", "--seed", "7"]) == 0
    (a, k), chk = seen[0], seen[1]
    assert a[5] == 3 and chk == ("check", 3)
    assert k == {"woa": None, "samples": 4, "sample_seed": 7}
    seen.clear()
    assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--samples=2"]) == 0
    assert seen[0][0][5] == -1 and seen[0][1] == {"woa": None, "samples": 2, "sample_seed": None}
    seen.clear()
    assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--seed", "9"]) == 0
    assert seen[0][1] == {"woa": None}                               # no --samples: infer is called as before
