"""Records tests/golden/encoder_vgpr_acc.npz: the rollout encoder's features of every case of tests/test_gpu_encoder_vgpr_acc.py, from
the PARENT of the commit that moved the encoder's MFMA accumulators to arch VGPRs.  Run once on the MI355X with the binding pointed at
the parent's library (a build of the parent commit, or of this tree's A/B arm):

    python 2048-ppo-agent_amd/build.py --encoder-agpr-acc /some/dir/libg2048.so
    G2048_LIB=/some/dir/libg2048.so python tests/golden/make_golden_encoder_vgpr_acc.py [OUT.npz]

Full f32 rows for B <= 23, sha256 of the rows' bytes above that, and the board pool the rows belong to.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (os.path.join(HERE, ".."), os.path.join(ROOT, "2048-ppo-agent_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import test_gpu_encoder_vgpr_acc as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    assert os.environ.get("G2048_LIB"), "point G2048_LIB at the parent's library"
    rows = T.compute(torch.device("cuda:0"))
    again = T.compute(torch.device("cuda:0"))
    store = {"boards": T.board_pool()}
    for case, v in rows.items():
        assert np.array_equal(v.view(np.uint32), again[case].view(np.uint32)), f"{case}: two runs differ"
        if v.shape[0] <= T.FULL_ROWS_MAX:
            store[case] = v
        else:
            store[case + "/sha256"] = np.array(T.digest(v))
    np.savez(out, **store)
    print(f"{out}: {len(rows)} cases, {os.path.getsize(out)} bytes")
