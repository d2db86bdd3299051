"""-m gpu: the fragment schedule of split_chain (csrc/coop_common.h) moves no arithmetic — the two production recurrent builds
(lstm_encode_coop_kernel<2,false,false>, pointer_decode_lean_kernel<true,2,EVH>) give, bit for bit, the arrays recorded from the
library of the commit before round 7 changed where the fragments are requested (profiles/LOG_r07.md;
tools/record_split_chain_prefetch.py; shapes and what each is there for: tests/golden/split_chain_prefetch_cases.py)."""
import pytest
import torch

from conftest import golden
import split_chain_prefetch_cases as cases

pytestmark = pytest.mark.gpu

FORMS = [pytest.param(wt, packed, id=f"{'write_through' if wt else 'same_xcd'}-{'packed' if packed else 'split_in_kernel'}")
         for wt in (False, True) for packed in (True, False)]


@pytest.fixture(scope="module")
def recorded():
    return golden(cases.ENC_FIXTURE), golden(cases.DEC_FIXTURE)


def same(got, want):
    want = torch.from_numpy(want)
    got = torch.from_numpy(got)
    return got.dtype == want.dtype and torch.equal(got.view(torch.int32), want.view(torch.int32))   # bit patterns (R of an all-dummy row may be NaN)


@pytest.mark.parametrize("write_through,packed", FORMS)
@pytest.mark.parametrize("L", cases.ENC_LENGTHS)
def test_encoder_bits_unchanged(dev, recorded, L, write_through, packed):
    fx = recorded[0]
    r = cases.run_encoder(dev, L, torch.from_numpy(fx[cases.enc_key(L, "x")]), write_through, packed)
    assert same(r["enc_out"], fx[cases.enc_key(L, "enc_out")])
    assert same(r["h_n"], fx[cases.enc_key(L, "enc_out")][:, :, L - 1].copy())
    assert same(r["c_n"], fx[cases.enc_key(L, "c_n")])


@pytest.mark.parametrize("write_through,packed", FORMS)
@pytest.mark.parametrize("T,K", cases.DEC_SHAPES)
def test_decoder_bits_unchanged(dev, recorded, T, K, write_through, packed):
    fx = recorded[1]
    r = cases.run_decoder(dev, T, K, torch.from_numpy(fx[cases.dec_key(T, K, "x")]), write_through, packed)
    for k in ("enc_rows", "enc_bits", "h_n", "c_n", "idx_low", "idx_high", "win_low", "win_high_raw", "R", "actions", "action_probs"):
        assert same(r[k], fx[cases.dec_key(T, K, k)]), k
