"""Chunk-masked encoder attention, host side (no GPU): the mask's definition, the configuration rules, the dynamic-chunk draw and the
argument checks of asr_sdpa_chunk_fwd / asr_sdpa_chunk_bwd through both call paths."""
import pytest
import torch

from tests import chunk_ref as CR


@pytest.mark.parametrize("T,C,left", [(1, 1, -1), (7, 1, -1), (7, 3, -1), (7, 3, 0), (7, 3, 1), (20, 4, 2), (20, 5, 0), (13, 16, -1),
                                      (13, 13, 2), (30, 7, 10)])
def test_mask_formula_matches_the_loop(T, C, left):
    assert torch.equal(CR.chunk_visible(T, T, C, left), CR.chunk_visible_loop(T, T, C, left))


def test_mask_special_cases():
    T = 11
    full = torch.ones(T, T, dtype=torch.bool)
    causal = torch.tril(full)
    for C in (T, T + 1, 100):
        assert torch.equal(CR.chunk_visible(T, T, C, -1), full)
        assert torch.equal(CR.chunk_visible(T, T, C, 0), full)          # one chunk: no left context needed
    assert torch.equal(CR.chunk_visible(T, T, 1, -1), causal)
    assert torch.equal(CR.chunk_visible(T, T, 1, 0), torch.eye(T, dtype=torch.bool))
    # key lengths: a query past the left context of every valid key sees nothing
    vis = CR.chunk_visible(12, 12, 4, 0, k_len=[12, 5, 0])
    assert vis[0].any(-1).all()
    assert vis[1, :8].any(-1).all() and not vis[1, 8:].any()
    assert not vis[2].any()


def _model(**over):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = Models.TransformerCTC
    mc = M.get_default_config()()
    mc.fn_build(dict(dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=1, n_mels=8, lfr_m=1, ctc_weight=1.0), **over))
    return M(mc, Vocab.synthetic(20))


def test_config_defaults_and_validation():
    m = _model()
    assert (m.chunk_size, m.left_chunks, m.encoder_mask(True), m.encoder_mask(False)) == (0, -1, (0, -1), (0, -1))
    m = _model(chunk_size=16, left_chunks=2)
    assert m.encoder_mask(True) == (16, 2) and m.encoder_mask(False) == (16, 2)       # decoding follows a static chunk
    m = _model(chunk_size=16, decoding_chunk_size=8, decoding_left_chunks=-1)
    assert m.encoder_mask(False) == (8, -1)
    m = _model(chunk_size=-1)
    assert m.encoder_mask(False) == (0, -1)                                           # dynamic training: full attention by default
    assert _model(chunk_size=-1, decoding_chunk_size=4).encoder_mask(False) == (4, -1)
    with pytest.raises(ValueError):
        _model(chunk_size=16, attn_window=50)
    with pytest.raises(ValueError):
        _model(chunk_size=-1, attn_window=50)
    with pytest.raises(ValueError):
        _model(decoding_chunk_size=8, attn_window=50)
    with pytest.raises(ValueError):
        _model(chunk_size=-2)
    with pytest.raises(ValueError):
        _model(left_chunks=-3)


def test_dynamic_chunk_is_a_pure_function_of_the_step():
    from asr_chinese_e2e_amd.Models.transformer_official import TransformerCTC as M
    draws = [M.dynamic_chunk(s) for s in range(4000)]
    assert draws == [M.dynamic_chunk(s) for s in range(4000)]
    full = sum(d == 0 for d in draws) / len(draws)
    assert 0.45 < full < 0.55                                          # full attention half the time
    chunks = [d for d in draws if d]
    assert min(chunks) == 1 and max(chunks) == M.DYN_CHUNK_MAX == 25
    assert len(set(chunks)) == 25
    m = _model(chunk_size=-1, left_chunks=3)
    for s in (1, 2, 3, 17, 1000):
        m._step_seed = s
        C = M.dynamic_chunk(s)
        assert m.encoder_mask(True) == ((C, 3) if C else (0, -1))


def test_graphed_step_refuses_dynamic_chunk():
    from asr_chinese_e2e_amd.graph import GraphedStep
    from asr_chinese_e2e_amd.Utils import Pack

    class Opt:
        def fused_step(self, *a):
            pass
    m = _model(chunk_size=-1)
    m.train()
    with pytest.raises(ValueError, match="dynamic chunk"):
        GraphedStep(m, Opt(), Pack(wave=torch.zeros(1, 4, 8), wave_len=torch.tensor([4])))


@pytest.mark.parametrize("path", ["ctypes", "fastcall"])
@pytest.mark.parametrize("chunk,left", [(0, -1), (-5, -1), (4, -2), (1, -7)])
def test_entry_points_reject_bad_chunk_arguments_without_gpu(path, chunk, left):
    from asr_chinese_e2e_amd import _lib
    f = _lib.lib if path == "ctypes" else _lib.fast
    rc = f.asr_sdpa_chunk_fwd(None, None, None, None, None, None, 2, 4, 16, 16, 64, 256, 256, 256, 256, chunk, left, 0.125, 0.0, 0,
                              None, _lib.ASR_BF16, None)
    assert rc == -1 and f"chunk={chunk} left_chunks={left}" in _lib.last_error()
    rc = f.asr_sdpa_chunk_bwd(None, None, None, None, None, None, None, 1024, None, None, None, None, 2, 4, 16, 16, 64, 256, 256, 256,
                              256, chunk, left, 0.125, 0.0, 0, None, _lib.ASR_BF16, None)
    assert rc == -1 and f"chunk={chunk} left_chunks={left}" in _lib.last_error()


def test_entry_points_check_pointers_after_a_valid_chunk():
    from asr_chinese_e2e_amd import _lib
    for f in (_lib.lib, _lib.fast):
        assert f.asr_sdpa_chunk_fwd(None, None, None, None, None, None, 2, 4, 16, 16, 64, 256, 256, 256, 256, 4, 1, 0.125, 0.0, 0,
                                    None, _lib.ASR_BF16, None) == -1
        assert "asr_sdpa_chunk_fwd: null pointer" in _lib.last_error()
        assert f.asr_sdpa_chunk_bwd_workspace_bytes(2, 4, 16, 20, 64, 4, 1, _lib.ASR_BF16) == 2 * 4 * 16 * 4
