"""Record the fixtures of tests/test_gpu_split_chain_prefetch.py: run on the GPU AT THE COMMIT WHOSE RESULTS ARE THE REFERENCE
(the parent of a change to split_chain's fragment schedule), with the library built.

    python tools/record_split_chain_prefetch.py [golden_dir]     (default: tests/golden; writes split_chain_prefetch/{enc,dec}.npz)

Every case also runs in the other three forms (write-through hand-off, weights split in the kernel) and must give the same bits
before anything is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import split_chain_prefetch_cases as cases   # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    dev = torch.device("cuda:0")
    enc, dec = cases.record(dev)
    for wt in (False, True):
        for packed in (True, False):
            for L in cases.ENC_LENGTHS:
                r = cases.run_encoder(dev, L, torch.from_numpy(enc[cases.enc_key(L, "x")]), wt, packed)
                assert np.array_equal(r["enc_out"], enc[cases.enc_key(L, "enc_out")]) and np.array_equal(r["c_n"], enc[cases.enc_key(L, "c_n")]), (L, wt, packed)
            for T, K in cases.DEC_SHAPES:
                r = cases.run_decoder(dev, T, K, torch.from_numpy(dec[cases.dec_key(T, K, "x")]), wt, packed)
                for k, v in r.items():
                    assert np.array_equal(v, dec[cases.dec_key(T, K, k)], equal_nan=True), (T, K, k, wt, packed)
    os.makedirs(os.path.join(out_dir, cases.FIXTURE_DIR), exist_ok=True)
    np.savez(os.path.join(out_dir, cases.ENC_FIXTURE), **enc)
    np.savez(os.path.join(out_dir, cases.DEC_FIXTURE), **dec)
    for name in (cases.ENC_FIXTURE, cases.DEC_FIXTURE):
        print(name, os.path.getsize(os.path.join(out_dir, name)), "bytes")


if __name__ == "__main__":
    main()
