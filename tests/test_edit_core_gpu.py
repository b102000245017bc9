"""The users of csrc/edit_wave.h's forward pass are one function: asr_edit_align in counts mode and in ops mode, asr_mwer_errors and the
pair_dist stage of asr_nbest_consensus give the same distance, integer for integer, and it is the definition's (tests/score_ref.py).  All
64 ordered (reference length, hypothesis length) pairs of LENS - 255 is the MWER limit, 63 / 64 / 65 / 128 / 129 the edges of the column
blocks and of the v_readlane row blocks - for an alphabet with ties in every cell and for the full vocabulary: one launch per source."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import score_ref as R  # noqa: E402

DEV = "cuda"
LENS = (0, 1, 63, 64, 65, 128, 129, 255)
L = max(LENS)


@pytest.mark.parametrize("V", [2, 4232])
def test_four_sources_one_distance(V):
    from asr_chinese_e2e_amd import kernels as K
    rng = np.random.default_rng(V)
    shapes = [(m, n) for m in LENS for n in LENS]
    P = len(shapes)
    ref, hyp = np.zeros((P, L), dtype=np.int32), np.zeros((P, L), dtype=np.int32)
    for p, (m, n) in enumerate(shapes):
        ref[p, :m] = rng.integers(0, V, m)
        hyp[p, :n] = rng.integers(0, V, n)
    ref_len, hyp_len = np.array([s[0] for s in shapes], dtype=np.int32), np.array([s[1] for s in shapes], dtype=np.int32)
    want = np.array([R.table(ref[p, :m], hyp[p, :n])[m, n] for p, (m, n) in enumerate(shapes)], dtype=np.int64)

    d = lambda a: torch.from_numpy(a).to(DEV)
    ref_d, hyp_d, ref_len_d, hyp_len_d = d(ref), d(hyp), d(ref_len), d(hyp_len)
    ref_of = np.arange(P, dtype=np.int32)
    got = {}
    for ops in (False, True):
        counts, _, n_ops = K.edit_align(hyp_d, hyp_len_d, ref_d, ref_len_d, d(ref_of), hyp_len, ref_len, ref_of, ops=ops)
        got["edit_align ops" if ops else "edit_align counts"] = counts[:, 0]
        if ops:
            assert (n_ops >= 0).all()      # every pair had its direction masks
    err, flags = K.mwer_errors(hyp_d.view(P, 1, L), hyp_len_d.view(P, 1), ref_d, ref_len_d)
    assert not flags.any()
    got["mwer_errors"] = err.view(P)
    # entry 0 is the row side of the pair (0, 1): the reference
    tok, ln = torch.stack([ref_d, hyp_d], dim=1).contiguous(), torch.stack([ref_len_d, hyp_len_d], dim=1).contiguous()
    host_ln, ones = np.stack([ref_len, hyp_len], axis=1), np.ones((P, 2), dtype=np.int32)
    out = K.nbest_consensus(tok, ln, d(ones), host_ln, ones, alts=1, stage="pair_dist")
    dist = K.nbest_unpack(out, P, 2, L, 1)["d"]
    assert (dist[:, 0, 1] == dist[:, 1, 0]).all() and not dist[:, 0, 0].any() and not dist[:, 1, 1].any()
    got["nbest pair_dist"] = dist[:, 0, 1]

    for name, g in got.items():
        g = g.cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(g != want)
        assert bad.size == 0, (name, [(shapes[p], int(g[p]), int(want[p])) for p in bad[:8]])
