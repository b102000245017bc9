"""Independent sessions on the GPU: the new kernels against their neighbours and tests/session_ref.py, then model.sessions against
model.stream - bit for bit where a slot is fed what a lock-step utterance is fed, within test_streaming_equals_offline's gates
against a B = 1 stream - audio through the independent front end, and endpointing at model level.

The model is tests/test_chunk_gpu.py's tiny one (d_model 64, 4 heads of 16, 2 layers, V = 30, C = 8, F = 16); one bf16 case at
dk = 64, C = 16 reaches the MFMA attention kernels."""
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import session_ref as SR  # noqa: E402

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


# ================================================================================================ kernels
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 100, 512])
def test_add_ln_slots_fwd_has_add_ln_fwds_bits(K, d, dtype):
    g = torch.Generator().manual_seed(d)
    pe_rows = 40
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    pe = torch.randn(pe_rows, d, generator=g).to(DEV)
    for S, C in ((4, 8), (1, 8), (3, 1), (5, 7)):
        x = (torch.randn(S * C, d, generator=g) * 2 + 0.3).to(DT[dtype]).to(DEV)
        # equal offsets: asr_add_ln_fwd with the table starting at that row
        off = 13
        lens = [C, 0, max(1, C // 2), C, C - 1][:S]
        want, _, _ = K.add_ln_fwd(x.clone(), None, gamma, beta, pe[off:], _i32(lens), S, C)
        got = K.add_ln_slots_fwd(x.clone(), gamma, beta, pe, _i32([off] * S), [off] * S, _i32(lens), S, C)
        assert torch.equal(got, want), (S, C, "equal offsets")
        # distinct offsets (one ends exactly at the table's last row): asr_add_ln_fwd on one utterance of S * C rows with a gathered table
        offs = [pe_rows - C, 0, 5, 17, 3][:S]
        table = torch.cat([pe[o:o + C] for o in offs])
        want, _, _ = K.add_ln_fwd(x.clone(), None, gamma, beta, table, None, 1, S * C)
        want = want.view(S, C, d).clone()
        for b, l in enumerate(lens):
            want[b, l:] = 0
        got = K.add_ln_slots_fwd(x.clone(), gamma, beta, pe, _i32(offs), offs, _i32(lens), S, C)
        assert torch.equal(got.view(S, C, d), want), (S, C, "distinct offsets")
        assert bool((got.view(S, C, d)[0] != 0).any()) or lens[0] == 0
    with pytest.raises(ValueError, match="positional table"):
        K.add_ln_slots_fwd(x, gamma, beta, pe, _i32([0] * 5), [0, 0, pe_rows - 6, 0, 0], _i32([7] * 5), 5, 7)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_slot_rows_put_and_slide_match_indexing(K, dtype):
    g = torch.Generator().manual_seed(9)
    S, C, cap, hd = 5, 8, 24, 64
    for case, (start, n) in enumerate([([0, 16, 3, 8, 1], [8, 8, 5, 0, 1]), ([0, 0, 9, 0, 0], [0, 0, 8, 0, 0]), ([16, 15, 0, 23, 2], [8, 8, 8, 1, 3])]):
        qkv = torch.randn(S * C, 3 * hd, generator=g).to(DT[dtype]).to(DEV)
        dst = torch.randn(S, cap, 2 * hd, generator=g).to(DT[dtype]).to(DEV)
        want = dst.clone()
        for b in range(S):
            want[b, start[b]:start[b] + n[b]] = qkv[b * C:b * C + n[b], hd:]
        got = K.slot_rows_put(qkv[:, hd:], dst, _i32(start), _i32(n), C)      # source rows are a column slice
        assert torch.equal(got, want), case
    # a row that would leave the window is dropped, the neighbour slot keeps every byte
    dst = torch.zeros(2, 8, 2 * hd, dtype=DT[dtype], device=DEV)
    src = torch.ones(2 * 8, 2 * hd, dtype=DT[dtype], device=DEV)
    K.slot_rows_put(src, dst, _i32([5, 0]), _i32([8, 0]), 8)
    assert bool((dst[0, 5:] == 1).all()) and bool((dst[0, :5] == 0).all()) and bool((dst[1] == 0).all())
    for case, (frm, cnt) in enumerate([([8, 0, 3, 0, 24 - 16], [16, 5, 16, 0, 16]), ([0] * 5, [0] * 5), ([1, 2, 3, 4, 5], [1, 16, 0, 7, 16])]):
        src = torch.randn(S, cap, 2 * hd, generator=g).to(DT[dtype]).to(DEV)
        dst = torch.randn(S, cap, 2 * hd, generator=g).to(DT[dtype]).to(DEV)
        want = dst.clone()
        for b in range(S):
            want[b, :cnt[b]] = src[b, frm[b]:frm[b] + cnt[b]]
        assert torch.equal(K.slot_rows_slide(src, dst, _i32(frm), _i32(cnt), 16), want), case


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [2, 30, 4232, 4233])
def test_ctc_frame_best_blank_is_argmax_and_topks_blank(K, V, dtype):
    from tests.test_decode_kernels_gpu import _lp_tol
    g = torch.Generator().manual_seed(V)
    for R in (1, 5, 257):
        x = torch.randn(R, V, generator=g) * 3
        x[R // 2] = torch.randint(0, 3, (V,), generator=g).float()      # ties in the maximum: the first wins
        if R > 2:
            x[1] = (3.0 + 0.01 * torch.randn(V, generator=g))              # in bf16 these collapse onto a few values
            x[2, V - 1] = x[2].max() + 1                                       # the maximum in the scalar tail / last vector
        x = x.to(DT[dtype])
        xd = x.to(DEV)
        path, blp = K.ctc_frame_best_blank(xd.view(1, R, V), None, 0)
        want_path = K.ctc_frame_argmax(xd.view(1, R, V), _i32([R]), 0)
        _, _, want_blp = K.ctc_frame_topk(xd, min(V, 4), 0)
        assert torch.equal(path, want_path)
        assert torch.equal(blp.view(-1), want_blp)
        ref_path, ref_blp = SR.frame_best_blank(x.double().numpy(), 0)
        assert np.array_equal(path.view(-1).cpu().numpy(), ref_path)
        x64 = x.double().numpy()
        m = x64.max(axis=1)
        lse = m + np.log(np.exp(x64 - m[:, None]).sum(axis=1))
        tol = _lp_tol(x64[:, :1], lse, V)[:, 0]
        assert (np.abs(blp.view(-1).double().cpu().numpy() - ref_blp) <= tol).all()
    # frames past in_len: asr_ctc_frame_argmax's blank, log p = 0; rows padded to ld > V are not read past V
    buf = torch.full((6, V + 3), 3.0e38).to(DT[dtype])
    buf[:, :V] = x[:1].expand(6, V) if x.shape[0] < 6 else x[:6]
    xd = buf.to(DEV)[:, :V].view(2, 3, V)
    lens = _i32([2, 0])
    path, blp = K.ctc_frame_best_blank(xd, lens, 0)
    assert torch.equal(path, K.ctc_frame_argmax(xd, lens, 0))
    assert path[1].tolist() == [0, 0, 0] and blp[1].tolist() == [0.0, 0.0, 0.0] and blp[0, 2].item() == 0.0
    assert torch.isfinite(blp).all()


@pytest.mark.parametrize("C", [1, 5, 8])
def test_session_ctc_step_matches_the_definition(K, C):
    """Logits with p(blank) = 0.5 or 0.95 (float64 check: every frame is at least 0.1 from the 0.8 threshold, no rounding can flip
    it) through asr_ctc_frame_best_blank; the classes are drawn independently (repeats, blanks) so the collapse has work to do.
    The frames are cut into chunks of C with ticks sat out in between and a reset in the middle."""
    S, T, V = 3, 41, 6
    rng = random.Random(C)
    p_blank = [[rng.choice([0.5, 0.95]) for _ in range(2 * T)] for _ in range(S)]
    cls = [[rng.choice([0, 0, 1, 1, 2, 3]) for _ in range(2 * T)] for _ in range(S)]
    thr, silence_lp = 0.8, math.log(0.8)

    def logits_of(p):      # blank = log p, one other class takes the rest
        row = [-80.0] * V
        row[0], row[1] = math.log(p), math.log(1 - p)
        return row
    state = torch.zeros(S, 4, dtype=torch.int32, device=DEV)
    ref_state = [None] * S
    pos, lim = [0] * S, [T] * S      # each slot reads on along its tape of 2 T frames up to lim
    fresh = [True] * S
    reopened = False
    emitted = 0
    for tick in range(400):
        if all(p >= l for p, l in zip(pos, lim)):
            break
        if not reopened and pos[1] >= 17:      # slot 1 is reopened in the middle: a second session of 20 frames
            reopened, fresh[1], lim[1] = True, True, pos[1] + 20
        rs = [int(f) for f in fresh]
        nv = [min(C, lim[b] - pos[b]) if pos[b] < lim[b] and rng.random() < 0.7 else 0 for b in range(S)]      # 0: the slot sits the tick out
        rows_l, rows_p = [], []
        for b in range(S):
            for t in range(C):
                i = min(pos[b] + t, 2 * T - 1)
                rows_l.append(logits_of(p_blank[b][i]))
                rows_p.append(cls[b][i])
        x = torch.tensor(rows_l, dtype=torch.float32)
        p64 = torch.softmax(x.double(), -1)[:, 0]
        assert float((p64 - thr).abs().min()) >= 0.1
        _, blp = K.ctc_frame_best_blank(x.to(DEV).view(S, C, V), None, 0)
        path = torch.tensor(rows_p, dtype=torch.int32, device=DEV).view(S, C)
        out = K.session_ctc_step(path, blp, _i32(nv), _i32(rs), state, C, silence_lp, 0).cpu().tolist()
        blp_h = blp.cpu().numpy()
        st_h = state.cpu().tolist()
        for b in range(S):
            ids, new = SR.ctc_step(rows_p[b * C:(b + 1) * C], blp_h[b], nv[b], bool(rs[b]), ref_state[b], silence_lp, 0)
            assert out[b][0] == len(ids) and out[b][4:4 + len(ids)] == ids and out[b][4 + len(ids):] == [0] * (C - len(ids)), (tick, b)
            assert tuple(out[b][1:4]) == new[1:] and tuple(st_h[b]) == new, (tick, b, out[b], new)
            ref_state[b] = new
            emitted += len(ids)
            pos[b] += nv[b]
            fresh[b] = False
    assert emitted > 0 and reopened and pos == lim
    # beam sessions: no path - nothing emitted, last and decoded kept, the counters run
    before = state.cpu().tolist()
    out = K.session_ctc_step(None, blp, _i32([C, 0, C]), _i32([0, 0, 0]), state, C, silence_lp, 0).cpu().tolist()
    after = state.cpu().tolist()
    for b in (0, 2):
        ids, new = SR.ctc_step(None, blp_h[b], C, False, tuple(before[b]), silence_lp, 0)
        assert out[b][0] == 0 and tuple(after[b]) == new
    assert after[1] == before[1]


def test_prefix_beam_state_reset_touches_only_the_flagged_slot(K):
    B, C, V, beam, k, T_cap = 3, 8, 12, 4, 5, 64
    g = torch.Generator().manual_seed(21)
    chunks = [torch.randn(B * C, V, generator=g).to(DEV) * 2 for _ in range(6)]
    st = K.ctc_prefix_beam_state(B, beam, T_cap, DEV)
    for x in chunks[:3]:
        K.ctc_prefix_beam_chunk(st, *K.ctc_frame_topk(x, k, 0), [C, C - 3, C], C, beam)
    state0, ws0 = st.state.clone(), st.ws.clone()
    K.ctc_prefix_beam_state_reset(st, _i32([0, 1, 0]), [1])
    per = st.state.numel() // B
    nodes = st.ws.view(torch.int32).view(B, -1)
    nodes0 = ws0.view(torch.int32).view(B, -1)
    for b in (0, 2):
        assert torch.equal(st.state.view(B, per)[b], state0.view(B, per)[b]) and torch.equal(nodes[b], nodes0[b])
    fresh = K.ctc_prefix_beam_state(B, beam, T_cap, DEV)
    assert torch.equal(st.state.view(B, per)[1], fresh.state.view(B, per)[1])      # byte for byte the initialised state
    assert st.frames == [3 * C, 0, 3 * C]
    for x in chunks[3:]:
        cand = K.ctc_frame_topk(x, k, 0)
        tok, ln, sc, stable = K.ctc_prefix_beam_chunk(st, *cand, [C, C, 0], C, beam, max_len=T_cap)
        tok2, ln2, sc2, stable2 = K.ctc_prefix_beam_chunk(fresh, *cand, [0, C, 0], C, beam, max_len=T_cap)
        assert torch.equal(ln[1], ln2[1]) and torch.equal(sc[1], sc2[1]) and torch.equal(tok[1], tok2[1]) and stable[1] == stable2[1]
    assert int(ln[1, 0]) > 0


# ================================================================================================ sessions against model.stream
_MODELS = {}


def _model(dtype, left, C=8, dk=16):
    from tests.test_chunk_gpu import _stream_model
    key = (dtype, left, C, dk)
    if key not in _MODELS:
        _MODELS[key] = _stream_model(dtype, left, C=C, dk=dk)
    return _MODELS[key]


def _feats(lens, dtype, seed, F=16):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(l, F, generator=g).to(DT[dtype]).to(DEV) for l in lens]


def _chunk_of(utts, pos, C, F=16):
    """(feats (n, C, F), n_valid): rows pos[i] .. pos[i] + C of each utterance (None: an empty slot), zero-padded."""
    some = next((u for u in utts if u is not None), None)      # nobody: a tick in which every slot sits out
    x = torch.zeros(len(utts), C, F, dtype=torch.float32 if some is None else some.dtype, device=DEV)
    nv = []
    for i, u in enumerate(utts):
        n = 0 if u is None else max(0, min(C, u.shape[0] - pos[i]))
        if n:
            x[i, :n] = u[pos[i]:pos[i] + n]
        nv.append(n)
    return x, nv


def _lockstep(model, utts, C, search, finish_kw=None):
    """model.stream(len(utts)) over the utterances side by side -> per utterance (encoder rows, ids, n-best), finish results."""
    st = model.stream(len(utts), search=search, beam_size=4, frame_topk=6)
    ids = [[] for _ in utts]
    per_push = []
    for c0 in range(0, max(u.shape[0] for u in utts), C):
        x, nv = _chunk_of(utts, [c0] * len(utts), C)
        got = st.push(x, nv)
        per_push.append((got, st.nbest() if search == "prefix_beam" else None))
        for b, g_ in enumerate(got):
            ids[b] += g_
    enc, lens = st.encoder_output()
    nbest = st.nbest() if search == "prefix_beam" else [None] * len(utts)
    fin = st.finish(**finish_kw) if finish_kw is not None else None
    return [(enc[b, :u.shape[0]].clone(), ids[b], nbest[b]) for b, u in enumerate(utts)], per_push, fin


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()))


def test_lockstep_stream_is_deterministic():
    """The forward path has no atomics: the bit-for-bit checks below rest on it."""
    model = _model("fp32", -1)
    utts = _feats([64, 61, 21, 6], "fp32", 3)
    a, _, _ = _lockstep(model, utts, 8, "greedy")
    b, _, _ = _lockstep(model, utts, 8, "greedy")
    for (ea, ia, _), (eb, ib, _) in zip(a, b):
        assert torch.equal(ea, eb) and ia == ib


@pytest.mark.parametrize("search", ["greedy", "prefix_beam"])
@pytest.mark.parametrize("left", [-1, 0, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sessions_in_lockstep_equal_the_stream_bit_for_bit(dtype, left, search):
    """model.stream is the lock-step view of model.sessions, so both sides run one tick: this pins the view's plumbing - every slot
    opened at construction, final = n_valid < C, the batch-list forms of nbest / encoder_output, a finish that frees nothing - against
    sessions driven by hand, no longer one implementation against another.  The independent oracles of the tick are the offline
    chunk-masked model (tests/test_chunk_gpu.py) and the offline prefix beam search (tests/test_stream_beam_gpu.py)."""
    C = 8
    model = _model(dtype, left)
    lens = [8 * C, 8 * C - 3, 2 * C + 5, C - 2]      # the unlimited cache grows past its first capacity; one ends inside its first chunk
    utts = _feats(lens, dtype, 3)
    finish_kw = dict(joint="ctc_rescore") if search == "prefix_beam" else dict(beam_size=3)
    want, per_push, want_fin = _lockstep(model, utts, C, search, finish_kw)
    ss = model.sessions(4, search=search, beam_size=4, frame_topk=6)
    for b in range(4):
        ss.open(b)
    for i, c0 in enumerate(range(0, max(lens), C)):
        x, nv = _chunk_of(utts, [c0] * 4, C)
        fin = [ss.state[b] == "open" and c0 + C >= lens[b] for b in range(4)]
        got = ss.push(x, nv, fin)
        assert got == per_push[i][0], (i, got, per_push[i][0])
        if search == "prefix_beam":
            assert [ss.nbest(b) for b in range(4)] == per_push[i][1], i
    assert [ss.status(b)["state"] for b in range(4)] == ["ended"] * 4 and [ss.status(b)["frames"] for b in range(4)] == lens
    assert ss.cap == {-1: 8 * C, 0: C, 2: 3 * C}[left] and len(ss.caches) == (1 if left < 0 else 2)      # model.stream's capacities
    enc, enc_lens = ss.encoder_output([0, 1, 2, 3])
    assert enc_lens.tolist() == lens
    for b in range(4):
        assert torch.equal(enc[b, :lens[b]], want[b][0]), b
        if search == "prefix_beam":
            assert ss.partial(b)["ids"] == want[b][2][0]["yseq"] and ss.partial(b)["score"] == want[b][2][0]["score"]
    got_fin = ss.finish([0, 1, 2, 3], **finish_kw)
    assert got_fin == want_fin
    assert any(r["ids"] for r in got_fin)
    assert [ss.status(b)["state"] for b in range(4)] == ["free"] * 4
    with pytest.raises(ValueError, match="free"):
        ss.push(x, [C, 0, 0, 0], [False] * 4)
    ss.open(0)
    ss.push(x, [0, 0, 0, 0], [True, False, False, False])      # closed without a frame: ended, the empty result
    assert ss.status(0)["state"] == "ended" and ss.finish(0, timestamps=False) == {"text": "", "ids": [], "score": float("-inf"), "tokens": None}
    with pytest.raises(ValueError, match="ended|free"):
        ss.finish(0)


def _sits(tick, b):
    """The fixed pseudo-random pattern of ticks a slot sits out."""
    return ((tick * 7 + b * 13 + 5) * 2654435761 >> 7) % 3 == 0


def _run_independent(model, utts, C, search, refuse=False):
    """Four slots, five utterances: slots start at different ticks and sit ticks out; utterance 2 (slot 2) ends inside its first chunk,
    is finished and the slot reopened in the same tick for utterance 4.  -> per utterance (encoder rows, ids, n-best), finish results."""
    ss = model.sessions(4, search=search, beam_size=4, frame_topk=6)
    start = [0, 1, 0, 2]
    in_slot = [0, 1, 2, 3]
    pos = [0] * 4
    ids = {u: [] for u in range(5)}
    res, fins = {}, {}
    table = model._ensure_engine(DEV).pe.shape[0]

    def close(b):
        u = in_slot[b]
        enc, ln = ss.encoder_output([b])
        assert ln.tolist() == [utts[u].shape[0]]
        res[u] = (enc[0, :utts[u].shape[0]].clone(), ids[u], ss.nbest(b) if search == "prefix_beam" else None)
        fins[u] = ss.finish(b, joint="ctc_rescore") if search == "prefix_beam" else ss.finish(b, beam_size=3)
        in_slot[b] = None
    for tick in range(64):
        for b in range(4):
            if tick == start[b]:
                ss.open(b)
        active = [in_slot[b] is not None and tick >= start[b] and ss.state[b] == "open" and not (_sits(tick, b) and tick > start[b]) for b in range(4)]
        x, nv = _chunk_of([utts[in_slot[b]] if active[b] else None for b in range(4)], pos, C)
        fin = [active[b] and pos[b] + C >= utts[in_slot[b]].shape[0] for b in range(4)]
        if refuse and tick >= 2 and any(active[b] and nv[b] == C for b in range(4)):
            refuse = False
            snap = (list(ss.state), list(ss.frames), list(ss.clen))
            b = next(b for b in range(4) if active[b] and nv[b] == C)
            with pytest.raises(ValueError, match="partial chunk"):
                ss.push(x, [C - 1 if i == b else n for i, n in enumerate(nv)], [False] * 4)
            keep, ss.frames[b] = ss.frames[b], table - C + 1
            with pytest.raises(ValueError, match="positional-encoding"):
                ss.push(x, nv, fin)
            ss.frames[b] = keep
            assert snap == (list(ss.state), list(ss.frames), list(ss.clen))
        got = ss.push(x, nv, fin)
        for b in range(4):
            if active[b]:
                ids[in_slot[b]] += got[b]
                pos[b] += nv[b]
            else:
                assert got[b] == []
        for b in range(4):
            if in_slot[b] is not None and ss.state[b] == "ended":
                first = in_slot[b] == 2
                close(b)
                if first:      # reopened in the same tick for the fifth utterance
                    ss.open(b)
                    in_slot[b], pos[b], start[b] = 4, 0, tick
        if all(u is None for u in in_slot):
            break
    assert sorted(res) == [0, 1, 2, 3, 4] and not refuse
    return res, fins


@pytest.mark.parametrize("search", ["greedy", "prefix_beam"])
@pytest.mark.parametrize("left", [-1, 0, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sessions_are_independent_of_their_neighbours(dtype, left, search):
    """Each utterance's encoder rows, ids and n-best equal, bit for bit, what it gets in the same slot of a lock-step model.stream(4)
    with other utterances beside it, and match a B = 1 stream within test_streaming_equals_offline's gates (fp32: 1e-4 max abs and
    equal ids; bf16: cosine 0.999).  The utterances have at most 4 chunks, so that with left = -1 the cache of every run keeps its
    first capacity (4 C rows) and the attention launches of the sessions and of the lock-step run have the same shape.  A refused
    push in the middle (a partial chunk without final, a push past the table) changes nothing of what follows."""
    C = 8
    model = _model(dtype, left)
    lens = [4 * C, 3 * C + 3, C - 3, 2 * C + 3, 2 * C + 6]
    utts = _feats(lens, dtype, 17)
    res, fins = _run_independent(model, utts, C, search)
    res2, fins2 = _run_independent(model, utts, C, search, refuse=True)
    finish_kw = dict(joint="ctc_rescore") if search == "prefix_beam" else dict(beam_size=3)
    # the same slot of a lock-step stream, other utterances beside it
    want_a, _, _ = _lockstep(model, [utts[0], utts[1], utts[2], utts[3]], C, search)
    want_b, _, _ = _lockstep(model, [utts[3], utts[0], utts[4], utts[1]], C, search)
    want = {0: want_a[0], 1: want_a[1], 2: want_a[2], 3: want_a[3], 4: want_b[2]}
    for u in range(5):
        for got, gfin in ((res[u], fins[u]), (res2[u], fins2[u])):
            assert torch.equal(got[0], want[u][0]), u
            assert got[1] == want[u][1] and got[2] == want[u][2], u
        assert fins[u] == fins2[u], u
    assert any(res[u][1] for u in range(5))
    # against B = 1
    for u in range(5):
        solo, _, fin1 = _lockstep(model, [utts[u]], C, search, finish_kw)
        a, r = res[u][0].float(), solo[0][0].float()
        if dtype == "fp32":
            assert float((a - r).abs().max()) <= 1e-4, (u, float((a - r).abs().max()))
            assert res[u][1] == solo[0][1] and fins[u]["ids"] == fin1[0]["ids"], u
        else:
            assert _cos(a, r) >= 0.999, (u, _cos(a, r))


def test_sessions_on_the_mfma_attention_kernels():
    """bf16, dk = 64, C = 16: staggered sessions through the MFMA key-length attention kernels against B = 1 streams."""
    C = 16
    model = _model("bf16", -1, C=C, dk=64)
    lens = [6 * C, 4 * C + 5, 3 * C - 1]
    utts = _feats(lens, "bf16", 23)
    ss = model.sessions(3)
    start, pos = [0, 2, 1], [0, 0, 0]
    for tick in range(12):
        for b in range(3):
            if tick == start[b]:
                ss.open(b)
        active = [ss.state[b] == "open" and not (_sits(tick, b) and tick > start[b]) for b in range(3)]
        x, nv = _chunk_of([utts[b] if active[b] else None for b in range(3)], pos, C)
        ss.push(x, nv, [active[b] and pos[b] + C >= lens[b] for b in range(3)])
        pos = [p + n for p, n in zip(pos, nv)]
    assert [ss.status(b)["state"] for b in range(3)] == ["ended"] * 3
    enc, _ = ss.encoder_output([0, 1, 2])
    for b in range(3):
        solo, _, _ = _lockstep(model, [utts[b]], C, "greedy")
        assert _cos(enc[b, :lens[b]].float(), solo[0][0].float()) >= 0.999, b


# ================================================================================================ audio
def _blocks(total, cuts):
    out, pos = [], 0
    for c in cuts:
        if pos >= total:
            break
        n = min(c, total - pos)
        out.append(n)
        pos += n
    assert pos == total
    return out


@pytest.mark.parametrize("frontend", ["reference", "kaldi"])
def test_push_audio_serves_every_slot_at_its_own_pace(frontend):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.data_handler.stream_frontend import StreamingFrontEnd
    C, S = 8, 3
    model = _model("fp32", 2)
    rng = np.random.default_rng(4)
    parser = AudioParser(n_mels=4, lfr_m=4, lfr_n=3, device=DEV, norm="global", cmvn=(rng.normal(-8, 1, 4), rng.uniform(0.2, 0.5, 4)), frontend=frontend)
    lens = [16000, 23111, 9000, 12345]      # the fourth takes slot 2 once the third has been finished
    wav = [(rng.standard_normal(l) * 0.1).astype(np.float32) for l in lens]
    r = random.Random(8)
    cuts = [_blocks(l, [r.choice([0, 480, 1600, 3000, 7680]) or 1 for _ in range(200)]) for l in lens]
    zero_blocks = {(0, 1), (1, 3), (2, 0)}      # (utterance, its block number): a zero-sample block is fed first
    # ---- the front end alone: each slot's feature rows are a B = 1 front end's
    fe = StreamingFrontEnd(parser, S, C, independent=True)
    rows = {u: [] for u in range(4)}
    in_slot, nxt, start = [0, 1, 2], [0, 0, 0], [0, 1, 3]
    done_u = set()
    for tick in range(400):
        ns, fin = [0] * S, [False] * S
        for b in range(S):
            u = in_slot[b]
            if u is None or tick < start[b] or fe.closed[b]:
                continue
            if (u, nxt[b]) in zero_blocks:
                zero_blocks.discard((u, nxt[b]))
                continue
            ns[b] = cuts[u][nxt[b]]
            nxt[b] += 1
            fin[b] = nxt[b] == len(cuts[u])
        pcm = torch.zeros(S, max(max(ns), 1))
        for b in range(S):
            if ns[b]:
                off = sum(cuts[in_slot[b]][:nxt[b] - 1])
                pcm[b, :ns[b]] = torch.from_numpy(wav[in_slot[b]][off:off + ns[b]])
        for feats, nv, done in fe.push_audio(pcm, ns, fin):
            for b in range(S):
                if nv[b]:
                    rows[in_slot[b]].append(feats[b, :nv[b]].clone())
                if done[b]:
                    done_u.add(in_slot[b])
                    if in_slot[b] == 2:
                        in_slot[b], nxt[b], start[b] = 3, 0, tick + 1
                        fe.reset(b)
                    else:
                        in_slot[b] = None
        if all(u is None for u in in_slot):
            break
    assert done_u == {0, 1, 2, 3}
    solo_rows = {}
    for u in range(4):
        one = StreamingFrontEnd(parser, 1, C)
        got = one.push_audio(torch.from_numpy(wav[u])[None], [lens[u]], [True])
        solo_rows[u] = torch.cat([f[0, :nv[0]] for f, nv in got if nv[0]])
        assert torch.equal(torch.cat(rows[u]), solo_rows[u]), u
    # ---- through the sessions: staggered opens, own block cuts; against a B = 1 stream with the same parser
    ss = model.sessions(S, parser=parser)
    ids = {u: [] for u in range(4)}
    enc, fins = {}, {}
    in_slot, nxt, start = [0, 1, 2], [0, 0, 0], [0, 1, 3]
    for tick in range(400):
        ns, fin = [0] * S, [False] * S
        for b in range(S):
            if in_slot[b] is not None and tick == start[b]:
                ss.open(b)
            u = in_slot[b]
            if u is None or tick < start[b] or ss.state[b] != "open":
                continue
            ns[b] = cuts[u][nxt[b]]
            nxt[b] += 1
            fin[b] = nxt[b] == len(cuts[u])
        pcm = torch.zeros(S, max(max(ns), 1))
        for b in range(S):
            if ns[b]:
                off = sum(cuts[in_slot[b]][:nxt[b] - 1])
                pcm[b, :ns[b]] = torch.from_numpy(wav[in_slot[b]][off:off + ns[b]])
        got = ss.push_audio(pcm if tick % 2 else pcm.to(DEV), ns, fin)
        for b in range(S):
            if in_slot[b] is not None:
                ids[in_slot[b]] += got[b]
            else:
                assert got[b] == []
            if in_slot[b] is not None and ss.state[b] == "ended":
                u = in_slot[b]
                e, ln = ss.encoder_output([b])
                assert ln.tolist() == [solo_rows[u].shape[0]]
                enc[u] = e[0, :solo_rows[u].shape[0]].clone()
                fins[u] = ss.finish(b, beam_size=3)
                in_slot[b] = None
                if u == 2:
                    in_slot[b], nxt[b], start[b] = 3, 0, tick + 1
        if all(u is None for u in in_slot):
            break
    assert sorted(enc) == [0, 1, 2, 3]
    for u in range(4):
        st = model.stream(1, parser=parser)
        want_ids = st.push_audio(torch.from_numpy(wav[u])[None], [lens[u]], [True])[0]
        e1, l1 = st.encoder_output()
        assert int(l1[0]) == enc[u].shape[0]
        assert float((enc[u].float() - e1[0, :int(l1[0])].float()).abs().max()) <= 1e-4, u
        assert ids[u] == want_ids and fins[u]["ids"] == st.finish(beam_size=3)[0]["ids"], u
    assert any(ids.values())
    # ---- fed in lock-step, everything equals model.stream(slots, parser=...) bit for bit: one tick under both, so this pins the
    # lock-step view's plumbing and the two front-end modes (independent or not) against each other
    st = model.stream(S, parser=parser)
    ss = model.sessions(S, parser=parser)
    for b in range(S):
        ss.open(b)
    tot_a, tot_b = [[] for _ in range(S)], [[] for _ in range(S)]
    block = 2000
    for off in range(0, max(lens[:S]), block):
        ns = [max(0, min(block, lens[b] - off)) for b in range(S)]
        fin = [0 < lens[b] - off <= block for b in range(S)]
        pcm = torch.zeros(S, block)
        for b in range(S):
            pcm[b, :ns[b]] = torch.from_numpy(wav[b][off:off + ns[b]])
        for b, (x, y) in enumerate(zip(st.push_audio(pcm, ns, fin), ss.push_audio(pcm, ns, fin))):
            tot_a[b] += x
            tot_b[b] += y
    assert tot_a == tot_b
    ea, la = st.encoder_output()
    eb, lb = ss.encoder_output(list(range(S)))
    assert la.tolist() == lb.tolist()
    for b in range(S):
        assert torch.equal(ea[b, :int(la[b])], eb[b, :int(la[b])]), b
    fa, fb = st.finish(beam_size=3), ss.finish(list(range(S)), beam_size=3)
    assert [r["ids"] for r in fa] == [r["ids"] for r in fb] and [r["score"] for r in fa] == [r["score"] for r in fb]
    with pytest.raises(ValueError, match="16 kHz"):
        model.sessions(2, parser=parser, source_rate=8000)


# ================================================================================================ endpointing at model level
@pytest.mark.parametrize("search", ["greedy", "prefix_beam"])
def test_endpoint_fires_at_the_frame_the_definition_gives(search):
    """Speech-like frames, then frames the model maps to blank (the blank row of the CTC head is set to separate the two kinds of
    encoder output).  After every tick the slot's counters and reported rule equal session_ref applied to the blank_lp values the
    kernel itself produced (float32 against the same float32 threshold on both sides); rule 2, shortened to 10 frames of silence,
    fires in the tick whose frames complete the run, not a chunk earlier.  A neighbour slot in a session of its own is not disturbed."""
    from tests.test_chunk_gpu import _stream_model
    C, n_speech, n_sil = 8, 20, 22
    g = torch.Generator().manual_seed(31)
    utt = torch.cat([torch.randn(n_speech, 16, generator=g), torch.full((n_sil, 16), 4.0) + 0.05 * torch.randn(n_sil, 16, generator=g)]).to(DEV)
    other = torch.randn(5 * C, 16, generator=g).to(DEV)
    probe = _model("fp32", -1)
    solo, _, _ = _lockstep(probe, [utt], C, "greedy")
    h = solo[0][0].double().cpu()
    w = h[n_speech:].mean(0) - h[:n_speech].mean(0)
    w = w / w.norm()
    proj = h @ w
    lo, hi = float(proj[:n_speech].max()), float(proj[n_speech:].min())
    assert hi - lo > 0.5, (lo, hi)      # the construction: the two kinds of frames are apart along w
    model = _stream_model("fp32", -1)
    sd = model.state_dict()
    alpha = 60.0 / (hi - lo)
    sd["ctc_lo.weight"][0] = (alpha * w).to(sd["ctc_lo.weight"].dtype)
    sd["ctc_lo.bias"][0] = float(-alpha * (hi + lo) / 2)
    model.load_state_dict(sd)
    frame_ms = model.frame_seconds() * 1000.0
    rule = (True, int(round(10 * frame_ms)), 0)
    ss = model.sessions(2, search=search, beam_size=4, frame_topk=6, endpoint={"silence_after_speech": rule})
    rules = ss.endpoint["rules"]
    assert abs(ss.frame_us - frame_ms * 1000) < 1e-6
    ss.open(0)
    state, fired_at, all_ids = None, None, []
    for tick, c0 in enumerate(range(0, utt.shape[0], C)):
        if tick == 1:
            ss.open(1)
        x, nv = _chunk_of([utt, other if tick >= 1 else None], [c0, max(0, c0 - C)], C)
        got = ss.push(x, nv, [c0 + C >= utt.shape[0], False])
        all_ids += got[0]
        blp = ss.last_blank_lp.view(2, C)[0].cpu().numpy()
        path = ss.last_path[0].cpu().tolist() if search == "greedy" else None
        ids, state = SR.ctc_step(path, blp, nv[0], tick == 0, state, math.log(0.8), 0)
        st = ss.status(0)
        assert (st["trailing_silence_frames"], st["frames"]) == (state[1], state[2]), tick
        decoded = bool(state[3]) if search == "greedy" else bool(ss.nbest(0)[0]["yseq"])
        if search == "greedy":
            assert got[0] == ids and st["decoded"] == decoded
        want = SR.endpoint_rule(state[1], state[2], decoded, ss.frame_us, rules)
        assert ss.endpoints()[0] == want, (tick, st, want)
        if want is not None and fired_at is None:
            fired_at = tick
        silent = blp[:nv[0]] > np.float32(math.log(0.8))
        assert silent.tolist() == [c0 + t >= n_speech for t in range(nv[0])], tick      # the construction held
    # silence starts at frame 20; its 10th frame is frame 29, in the fourth chunk (frames 24 .. 31)
    assert fired_at == 3 and ss.endpoints()[0] == "silence_after_speech" and (all_ids or search == "prefix_beam")
    assert ss.status(0)["state"] == "ended" and ss.status(1)["state"] == "open" and ss.status(1)["frames"] == 5 * C
    # the caller closes, finishes and reopens: the counters restart
    ss.finish(0, **(dict(joint="ctc_rescore") if search == "prefix_beam" else dict(beam_size=2)))
    ss.open(0)
    x, nv = _chunk_of([utt[n_speech + 2:], None], [0, 0], C)
    ss.push(x, nv, [False, False])
    blp = ss.last_blank_lp.view(2, C)[0].cpu().numpy()
    _, st2 = SR.ctc_step(ss.last_path[0].cpu().tolist() if search == "greedy" else None, blp, C, True, state, math.log(0.8), 0)
    assert st2[2] == C and (ss.status(0)["trailing_silence_frames"], ss.status(0)["frames"]) == (st2[1], st2[2]) and ss.endpoints()[0] is None
    assert ss.status(1)["frames"] == 5 * C


# ================================================================================================ command line
def test_transcribe_cli_sessions(tmp_path):
    """transcribe.py --stream=1 --sessions=2 on three short files: the final ids of every file are those of --stream=1 without
    --sessions, the per-chunk lines count each file's own chunks, and --endpoint=1 adds "endpoint" to them."""
    import json
    import os
    import subprocess
    import sys
    from asr_chinese_e2e_amd.data_handler import Vocab
    from asr_chinese_e2e_amd.data_handler.cmvn import save_cmvn
    from tests.helpers import ROOT
    from tests.test_ctc_align_gpu import _write_wav
    sys.path.insert(0, ROOT)
    from train import TrainConfig, get_model_class
    flags = dict(model_name="TransformerCTC", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32", n_mels=40,
                 decoding_chunk_size=8, decoding_left_chunks=2)
    config = TrainConfig()
    config.fn_build(flags)
    Model, MC = get_model_class(config.model_name)
    config.fn_combine(MC())
    config.fn_build(flags)
    vocab = Vocab.synthetic(40)
    vocab.save(str(tmp_path / "vocab.t"))
    torch.manual_seed(0)
    Model(config, vocab).save(str(tmp_path / "m.model"))
    save_cmvn(str(tmp_path / "cmvn.npz"), np.full(40, -6.0), np.full(40, 0.4), 1000)
    wavs = [tmp_path / "a.wav", tmp_path / "b.wav", tmp_path / "c.wav"]
    for i, (p, s) in enumerate(zip(wavs, [1.3, 0.5, 0.9])):
        _write_wav(p, s, i)
    base = [sys.executable, os.path.join(ROOT, "transcribe.py")] + [f"--{k}={v}" for k, v in flags.items()] + \
        [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}", "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3",
         f"--cmvn={tmp_path / 'cmvn.npz'}", "--stream=1"]
    runs = {}
    for name, extra in (("lockstep", []), ("sessions", ["--sessions=2", "--endpoint=1"])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        runs[name] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    final = {name: {l["file"]: l for l in lines if "ids" in l} for name, lines in runs.items()}
    assert sorted(final["sessions"]) == sorted(final["lockstep"]) == sorted(map(str, wavs))
    for f in final["lockstep"]:
        assert final["sessions"][f]["ids"] == final["lockstep"][f]["ids"] and final["sessions"][f]["text"] == final["lockstep"][f]["text"], f
        assert abs(final["sessions"][f]["duration_s"] - final["lockstep"][f]["duration_s"]) < 1e-9
    chunks = [l for l in runs["sessions"] if "chunk" in l]
    for f in map(str, wavs):
        mine = [l for l in chunks if l["file"] == f]
        assert [l["chunk"] for l in mine] == list(range(len(mine))) and mine and all("endpoint" in l for l in mine)
        assert [l["partial"] for l in mine] == [l["partial"] for l in runs["lockstep"] if "chunk" in l and l["file"] == f]
    order = [l["file"] for l in runs["sessions"] if "ids" in l]
    assert order.index(str(wavs[1])) < order.index(str(wavs[0]))      # in order of completion: the short second file ends first
    # c.wav took b.wav's slot while a.wav was still streaming
    first_c = next(i for i, l in enumerate(runs["sessions"]) if l["file"] == str(wavs[2]))
    last_a = max(i for i, l in enumerate(runs["sessions"]) if l["file"] == str(wavs[0]) and "chunk" in l)
    assert first_c < last_a
    r = subprocess.run([c for c in base if not c.startswith("--cmvn=")] + ["--sessions=2"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "--cmvn" in r.stderr
