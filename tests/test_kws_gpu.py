"""Keyword spotting on the GPU, bit for bit against its definition (tests/kws_ref.py): asr_kws_search + asr_kws_compact over dtypes, row
strides, vocabulary sizes, list sizes and lengths (every length bucket and the index map), -inf logits, exact ties, capacity; the
resumable asr_kws_chunk under every cutting against the offline call on the frames so far; model.spot_keywords, model.spot_long and
model.sessions / model.stream with keywords=.  Every comparison is of integers and float bits: there is no tolerance."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import kws_ref as R  # noqa: E402

DEV = "cuda"
MTF = 6      # max_token_frames of the kernel tests: frame_seconds 1.0, max_token_s 6.0


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _list(kws, ps, cap=8, max_hits=None):
    from asr_chinese_e2e_amd.keywords import KeywordList
    return KeywordList([(k, p) for k, p in zip(kws, ps)], max_token_s=float(MTF), hits_per_keyword=cap, max_hits=max_hits)


def _keywords(rng, V, K_, lengths):
    """K keywords over ids [1, V) with the given lengths in turn; every third one repeats a character somewhere (always when V = 2)."""
    out = []
    for k in range(K_):
        L = lengths[k % len(lengths)]
        w = [int(rng.integers(1, V)) for _ in range(L)]
        if L >= 2 and k % 3 == 0:
            i = int(rng.integers(1, L))
            w[i] = w[i - 1]
        out.append(w)
    return out


def _plant(rng, x, t, kw, gain=9.0):
    """Spell kw into rows x (T, V) from frame t on: each character 1-3 frames, sometimes a blank frame between two, always between
    equal ones.  Returns the frame behind the last one written."""
    T = x.shape[0]
    for i, c in enumerate(kw):
        if i and (kw[i - 1] == c or rng.random() < 0.4) and t < T:
            x[t, 0] += gain
            t += 1
        for _ in range(int(rng.integers(1, 4))):
            if t < T:
                x[t, c] += gain
                t += 1
    return t


def _case(seed, B, T, V, kws, in_len, plants=3, dtype=torch.float32, ld=None, neg_inf=False):
    """Random logits with keywords spelt into them, on the device as a (B, T, V) view of rows of stride ld."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (B, T, V)).astype(np.float32)
    for b in range(B):
        t = int(rng.integers(0, 4))
        for _ in range(plants):
            t = _plant(rng, x[b], t, kws[int(rng.integers(0, len(kws)))]) + int(rng.integers(1, 6))
        if in_len[b] > 0:      # a keyword that ends on the utterance's last frame: its run is still open there
            kw = kws[b % len(kws)]
            if kw[-1] != 0 and in_len[b] >= 2:
                x[b, in_len[b] - 2:in_len[b], :] = rng.normal(0.0, 1.0, (min(2, in_len[b]), V))
                x[b, in_len[b] - 2:in_len[b], kw[-1]] += 9.0
    if neg_inf:
        m = rng.random((B, T, V)) < 0.15
        m[:, :, 0] = False      # the blank stays finite, so no row is all -inf
        x[m] = -np.inf
    ld = V if ld is None else ld
    buf = torch.full((B * T, ld), float("nan"), dtype=dtype, device=DEV)      # the padding is poison: it is never read
    buf[:, :V] = torch.from_numpy(x).to(DEV).reshape(B * T, V).to(dtype)
    return buf.view(B, T, ld)[:, :, :V]


def _lp_lists(K, logits, in_len, lse=None):
    """(lse on the device, per utterance lp (in_len[b], V) float32 from the device's lse and the same logits bits)."""
    if lse is None:
        _, _, _, lse, _ = K.ctc_frame_stats(logits, _i32(in_len), 0)
    host, l = logits.float().cpu().numpy(), lse.cpu().numpy()
    return lse, [R.emissions(host[b, :n], l[b, :n]) for b, n in enumerate(in_len)]


def _check_search(K, logits, in_len, kws, ps, cap=8, max_hits=None, lse=None, want_dropped=None):
    kl = _list(kws, ps, cap, max_hits)
    lse, lps = _lp_lists(K, logits, in_len, lse)
    thr, span = [R.threshold(len(k), p) for k, p in zip(kws, ps)], [R.span_cap(len(k), float(MTF), 1.0) for k in kws]
    assert [np.float32(t) for t in kl.thr] == thr and kl.spans(1.0) == span
    want = R.search(lps, kws, thr, span)
    tabs = kl.on(DEV, 1.0)
    runs = [K.kws_search(logits, lse, _i32(in_len), tabs, kl.K, cap) for _ in range(2)]
    cnt, rec = (t.cpu().numpy() for t in runs[0])
    comp = [K.kws_compact(*r, kl.max_hits) for r in runs]
    count, dropped, hits = (t.cpu().numpy() for t in comp[0])
    total = 0
    for b in range(len(in_len)):
        wc, wr = R.capped(want[b], cap)
        assert np.array_equal(cnt[b], wc), (b, cnt[b], wc)
        assert np.array_equal(rec[b], wr), b
        n, dr, wh = R.compact(want[b], cap, kl.max_hits)
        assert (int(count[b]), int(dropped[b])) == (n, dr) and np.array_equal(hits[b], wh), b
        total += int(wc.sum())
    for a, b_ in zip(runs[0] + comp[0], runs[1] + comp[1]):      # the same bytes in every run
        assert torch.equal(a, b_)
    if want_dropped is not None:
        assert (dropped.sum() > 0) == want_dropped
    return want, total


# ------------------------------------------------------------------------------------------------ the offline kernel
@pytest.mark.parametrize("dtype, pad", [(torch.float32, 0), (torch.float32, 3), (torch.bfloat16, 0), (torch.bfloat16, 8)])
@pytest.mark.parametrize("V, K_, lengths", [
    (2, 1, [1]), (2, 5, [1, 2, 3, 16]),                                           # one token besides the blank: repeats only
    (5, 63, [1, 2, 4]), (5, 64, [5, 8]), (5, 65, [9, 16]),                        # one bucket each, at the edges of a wave
    (64, 130, [1, 2, 4, 5, 8, 9, 16]),                                            # every bucket in one list: three waves, the index map
])
def test_search_matches_the_definition(K, dtype, pad, V, K_, lengths):
    rng = np.random.default_rng(1000 * V + K_)
    kws = _keywords(rng, V, K_, lengths)
    ps = [float(rng.choice([0.2, 0.4, 0.6])) for _ in kws]
    in_len = [130, 57, 0]
    logits = _case(V + K_ + pad, 3, 130, V, kws, in_len, plants=5, dtype=dtype, ld=V + pad)
    want, total = _check_search(K, logits, in_len, kws, ps)
    assert total > 0 and not any(want[2][k] for k in range(K_))      # something is found; the empty utterance has no hit


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_search_one_utterance_short_lengths_and_the_wide_vocabulary(K, dtype):
    rng = np.random.default_rng(7)
    kws = _keywords(rng, 4232, 9, [2, 3, 6, 4, 5])
    for T, in_len in ((130, [130]), (1, [1]), (4, [3])):      # in_len = 1 and in_len < L: only the keywords that fit can hit
        logits = _case(T, 1, T, 4232, kws, in_len, dtype=dtype)
        _check_search(K, logits, in_len, kws, [0.3] * len(kws))
    one = [[5], [5, 5], [7, 5]]
    x = torch.zeros(1, 1, 16, device=DEV)
    x[0, 0, 5] = 12.0
    want, total = _check_search(K, x, [1], one, [0.5] * 3)
    assert total == 1 and [len(h) for h in want[0]] == [1, 0, 0] and want[0][0][0][:2] == (0, 0)


def test_search_with_minus_infinity_logits(K):
    rng = np.random.default_rng(3)
    kws = _keywords(rng, 12, 40, [1, 2, 3, 5, 9])
    in_len = [90, 33, 64]
    for dtype in (torch.float32, torch.bfloat16):
        logits = _case(5, 3, 90, 12, kws, in_len, plants=6, dtype=dtype, neg_inf=True)
        assert torch.isinf(logits.float()).any()
        _, total = _check_search(K, logits, in_len, kws, [0.3] * len(kws))
        assert total > 0


def test_exact_ties_on_a_grid_of_eighths(K):
    """Log-probabilities that are multiples of 1/8 with lse = 0: every sum is exact, so equal scores abound - stay against s-1 against
    s-2, and equal H inside a run (the first frame wins)."""
    rng = np.random.default_rng(17)
    B, T, V = 3, 80, 4
    x = -(rng.integers(0, 5, (B, T, V)) / 8.0).astype(np.float32)
    x[:, :, 0] = -0.125
    kws = [[1], [1, 2], [2, 2], [1, 2, 3], [3, 1, 1, 2], [1, 2, 3, 1, 2], [2, 1, 3, 2, 1, 3, 2, 1, 3]]
    logits = torch.from_numpy(x).to(DEV)
    lse = torch.zeros(B, T, device=DEV)
    in_len = [80, 41, 2]
    ps = [math.exp(-0.25)] * len(kws)      # thr = -L / 4: on the grid, so H == thr occurs
    want, total = _check_search(K, logits, in_len, kws, ps, cap=64, lse=lse)
    assert total > 20
    lp = x[0]
    H, _ = R.scan(lp, kws)
    thr = [R.threshold(len(k), p) for k, p in zip(kws, ps)]
    assert any((H[:, k] == thr[k]).any() for k in range(len(kws)))      # a candidate exactly on the threshold
    ties = sum(1 for k in range(len(kws)) for t in range(1, T) if H[t, k] == H[t - 1, k] and H[t, k] >= thr[k])
    assert ties > 0      # two neighbouring candidate frames of equal H


def test_capacity_counts_on_and_reports_dropped(K):
    kw = [[3, 4], [4], [9, 9]]
    T, V = 120, 12
    x = np.full((1, T, V), -4.0, dtype=np.float32)
    x[0, :, 0] = 4.0
    for i in range(11):      # "3 4" eleven times, a blank stretch between them
        x[0, 10 * i + 1, 3], x[0, 10 * i + 2, 4] = 9.0, 9.0
    logits = torch.from_numpy(x).to(DEV)
    want, _ = _check_search(K, logits, [T], kw, [0.5] * 3, cap=4, want_dropped=True)
    assert [len(h) for h in want[0]] == [11, 11, 0]
    kl = _list(kw, [0.5] * 3, cap=4)
    lse, _ = _lp_lists(K, logits, [T])
    count, dropped, hits = (t.cpu().numpy() for t in K.kws_compact(*K.kws_search(logits, lse, _i32([T]), kl.on(DEV, 1.0), 3, 4), kl.max_hits))
    assert int(count[0]) == 8 and int(dropped[0]) == 14
    assert hits[0, :8, 0].tolist() == [0] * 4 + [1] * 4 and hits[0, :4, 2].tolist() == [2, 12, 22, 32]      # the first cap, in order
    _check_search(K, logits, [T], kw, [0.5] * 3, cap=4, max_hits=5, want_dropped=True)      # the list's own limit drops three more
    _check_search(K, logits, [T], kw, [0.5] * 3, cap=16, want_dropped=False)


# ------------------------------------------------------------------------------------------------ the resumable form
class _Driver:
    """Feeds slots their frames in chunks of at most C through ctc_frame_stats + kws_chunk and keeps what every call emits."""

    def __init__(self, K, kl, logits, C, cap):
        self.K, self.kl, self.logits, self.C, self.cap = K, kl, logits, C, cap
        self.slots, _, self.V = logits.shape
        self.state = K.kws_state(self.slots, kl.K, DEV)
        self.at = [0] * self.slots          # frames of the source consumed
        self.base = [0] * self.slots        # the source frame a slot's session began on
        self.hits = [[[] for _ in range(kl.K)] for _ in range(self.slots)]
        self.tabs = kl.on(DEV, 1.0)

    def tick(self, n, reset=None, final=None, state=None, keep=True):
        reset, final = reset or [0] * self.slots, final or [0] * self.slots
        chunk = torch.full((self.slots, self.C, self.V), float("nan"), dtype=self.logits.dtype, device=DEV)
        for b in range(self.slots):
            if reset[b] and keep:
                self.base[b], self.hits[b] = self.at[b], [[] for _ in range(self.kl.K)]
            chunk[b, :n[b]] = self.logits[b, self.at[b]:self.at[b] + n[b]]
        _, _, _, lse, _ = self.K.ctc_frame_stats(chunk, _i32(n), 0)
        cnt, rec = self.K.kws_chunk(chunk, lse, _i32(n), _i32(reset), _i32(final), self.tabs, self.kl.K, self.state if state is None else state, self.cap)
        cnt, rec = cnt.cpu().numpy(), rec.cpu().numpy()
        assert (cnt <= self.cap).all()
        out = [[[tuple(int(v) for v in rec[b, k, i]) for i in range(cnt[b, k])] for k in range(self.kl.K)] for b in range(self.slots)]
        if keep:
            for b in range(self.slots):
                self.at[b] += n[b]
                for k in range(self.kl.K):
                    self.hits[b][k] += out[b][k]
        return out

    def offline(self, b):
        """asr_kws_search over slot b's frames so far, as per-keyword lists of (start, end, bits)."""
        n = self.at[b] - self.base[b]
        if n == 0:
            return [[] for _ in range(self.kl.K)]
        rows = self.logits[b:b + 1, self.base[b]:self.at[b]].contiguous()
        _, _, _, lse, _ = self.K.ctc_frame_stats(rows, _i32([n]), 0)
        cnt, rec = (t.cpu().numpy() for t in self.K.kws_search(rows, lse, _i32([n]), self.tabs, self.kl.K, 64))
        assert (cnt <= 64).all()
        return [[tuple(int(v) for v in rec[0, k, i]) for i in range(cnt[0, k])] for k in range(self.kl.K)]

    def closed_now(self, b):
        """The slot's hits if its input ended here: final on a copy of the state, no frames."""
        extra = self.tick([0] * self.slots, final=[1 if s == b else 0 for s in range(self.slots)], state=self.state.clone(), keep=False)
        return [self.hits[b][k] + extra[b][k] for k in range(self.kl.K)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cut", [1, 5, 16, 64, 65])
def test_any_cutting_gives_the_offline_hits(K, cut, dtype):
    rng = np.random.default_rng(cut)
    V, T, slots = 20, 130, 3
    kws = _keywords(rng, V, 70, [1, 2, 3, 5, 8, 9, 16])
    kl = _list(kws, [0.3] * len(kws), cap=16)
    logits = _case(11 + cut, slots, T, V, kws, [T] * slots, plants=6, dtype=dtype).contiguous()
    d = _Driver(K, kl, logits, 65, 16)
    tick = 0
    while min(d.at) < T:
        n = [min(cut, T - d.at[b]) for b in range(slots)]
        if tick % 3 == 1:
            n = [0] * slots                       # an empty chunk in between
        elif tick % 3 == 2:
            n[1] = 0                              # slot 1 sits every third tick out
        before = d.state.clone()
        d.tick(n)
        per = d.state.numel() // slots
        for b in range(slots):
            if n[b] == 0:
                assert torch.equal(before[b * per:(b + 1) * per], d.state[b * per:(b + 1) * per])      # untouched, every word
        if tick % 7 == 3:
            for b in range(slots):
                assert d.closed_now(b) == d.offline(b), (tick, b)
        tick += 1
    d.tick([0] * slots, final=[1] * slots)
    total = 0
    for b in range(slots):
        off = d.offline(b)
        assert d.hits[b] == off, b
        total += sum(len(h) for h in off)
    assert total > 10
    if cut == 1:      # every run of two candidate frames spans a chunk boundary
        _, lps = _lp_lists(K, logits, [T] * slots)
        H, hs = R.scan(lps[0], kws)
        thr = [R.threshold(len(k), 0.3) for k in kws]
        assert any(R.is_candidate(H[t, k], hs[t, k], t, thr[k], len(kws[k]) * MTF) and R.is_candidate(H[t + 1, k], hs[t + 1, k], t + 1, thr[k], len(kws[k]) * MTF)
                   for k in range(len(kws)) for t in range(T - 1))


def test_reset_in_mid_run_discards_the_open_run_and_final_closes_one(K):
    V, T = 8, 40
    kw = [[2, 3], [3]]
    x = np.full((2, T, V), -4.0, dtype=np.float32)
    x[:, :, 0] = 4.0
    for b in range(2):
        x[b, 4, 2], x[b, 5:9, 3] = 9.0, 9.0            # "2 3" with the 3 held over frames 5..8: a run of candidates
        x[b, 20, 2], x[b, 21:24, 3] = 9.0, 9.0
        x[b, T - 1, 3] = 9.0                            # a "3" on the last frame: open when the input ends
    logits = torch.from_numpy(x).to(DEV)
    kl = _list(kw, [0.5, 0.5], cap=8)
    d = _Driver(K, kl, logits, 8, 8)
    out = d.tick([7, 7])                                # frames 0..6: both runs are open, nothing is closed
    assert out == [[[], []], [[], []]]
    per = d.state.numel() // 2
    assert d.state[:per].view(-1)[(2 * 31) * 64] == 1   # slot 0, keyword row 0: the open flag of its run
    d.tick([8, 8], reset=[0, 1])                        # slot 1 starts again at frame 7: its open runs are gone, frames count from 0
    for _ in range(4):
        d.tick([8, 8] if d.at[0] + 8 <= T else [T - d.at[0]] * 2)
    assert d.at == [T, T] and d.base == [0, 7]
    open_before = [[list(h) for h in d.hits[b]] for b in range(2)]
    d.tick([0, 0], final=[1, 1])
    for b in range(2):
        assert d.hits[b] == d.offline(b)
        assert len(d.hits[b][1]) == len(open_before[b][1]) + 1 and d.hits[b][1][-1][:2] == (T - 1 - d.base[b], T - 1 - d.base[b])      # closed by final
    assert [h[:2] for h in d.hits[0][0]] == [(4, 5), (20, 21)] and [h[:2] for h in d.hits[1][0]] == [(13, 14)]
    # asr_kws_state_reset: the flagged slot is the initial state again, the other keeps every word
    fresh = K.kws_state(2, kl.K, DEV)
    before = d.state.clone()
    K.kws_state_reset(d.state, _i32([0, 1]), kl.K)
    assert torch.equal(d.state[per:], fresh[per:]) and torch.equal(d.state[:per], before[:per]) and not torch.equal(before[per:], fresh[per:])


# ------------------------------------------------------------------------------------------------ the model
def _want_hits(model, kl, logits, lse, in_len, b):
    """spot_keywords' hit list of utterance b from the definition over the model's own logits and the device's lse."""
    d = model.frame_seconds()
    lp = R.emissions(logits[b, :in_len[b]].float().cpu().numpy(), lse[b, :in_len[b]].cpu().numpy())
    per = R.search([lp], [list(i) for i in kl.ids], [np.float32(t) for t in kl.thr], kl.spans(d))[0]
    out = []
    for k, hits in enumerate(per):
        for s, e, sc in hits[:kl.hits_per_keyword]:
            out.append({"keyword": k, "phrase": "".join(model.vocab._id2token[x] for x in kl.ids[k]), "ids": list(kl.ids[k]), "start_frame": s, "end_frame": e,
                        "start_s": s * d, "end_s": (e + 1) * d, "score": float(sc), "confidence": math.exp(float(sc) / len(kl.ids[k]))})
    out.sort(key=lambda h: (h["end_frame"], h["keyword"]))
    return out, sum(max(0, len(h) - kl.hits_per_keyword) for h in per)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_spot_keywords_on_a_small_model(K, dtype):
    from asr_chinese_e2e_amd.Utils import Pack
    from asr_chinese_e2e_amd.keywords import KeywordList
    from tests.test_align_long_gpu import _model
    model = _model(dtype)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(3, 70, 320, generator=g).to(DEV)
    in_len = [70, 41, 9]
    pack = Pack(wave=feats, wave_len=_i32(in_len))
    logits = model._ctc_logits(pack)
    path, _, _, lse, _ = K.ctc_frame_stats(logits, _i32(in_len), 0)
    words = []
    for b, n in enumerate(in_len):      # what the best path spells, in pieces of one to three characters
        p = path[b, :n].cpu().tolist()
        seq = [c for i, c in enumerate(p) if c != 0 and (i == 0 or c != p[i - 1])]
        words += [seq[i:i + m] for m in (1, 2, 3) for i in range(0, max(0, len(seq) - m + 1), 2)]
    words = [w for w in words if w][:50] + [[4, 4], [5, 6, 7, 8, 9], [29] * 16]
    kl = KeywordList(words, threshold=0.3, vocab_size=30, hits_per_keyword=3)
    got = model.spot_keywords(pack, kl)
    assert len(got) == 3 and sum(len(r["hits"]) for r in got) > 5
    for b in range(3):
        want, dropped = _want_hits(model, kl, logits, lse, in_len, b)
        assert got[b]["hits"] == want and got[b]["dropped"] == dropped
    assert logits.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32)


# ------------------------------------------------------------------------------------------------ sessions and the lock-step stream
def _session_keywords(model, utts):
    """Phrases of one to three characters cut from the offline best paths (so that some are found), a doubled one, a long one."""
    from asr_chinese_e2e_amd.Utils import Pack
    from asr_chinese_e2e_amd.keywords import KeywordList
    words = []
    for u in utts:
        seq = model.ctc_greedy_search(Pack(wave=u[None], wave_len=_i32([u.shape[0]])))[0]
        words += [seq[i:i + m] for m in (1, 2, 3) for i in range(0, max(0, len(seq) - m + 1), 2)]
    words = [w for w in words if w and 0 not in w][:60] + [[4, 4], [7] * 16]
    return KeywordList(words, threshold=0.25, max_token_s=0.3, vocab_size=30, hits_per_keyword=32, max_hits=1024)


def _drive(model, utts, C, kl, **kw):
    """Three slots, four utterances: slots start at different ticks and sit ticks out; the shortest utterance's slot is finished and
    reopened for the fourth.  -> (what every tick returned and reported, per utterance (hits, offline hits over the streamed rows))."""
    from asr_chinese_e2e_amd.Utils import Pack
    from tests.test_sessions_gpu import _chunk_of, _sits
    ss = model.sessions(3, endpoint={}, keywords=kl, **kw)
    start, in_slot, pos = [0, 1, 0], [0, 1, 2], [0, 0, 0]
    log, res = [], {}
    tick = 0
    while any(u is not None for u in in_slot):
        cur, fin = [], []
        for b in range(3):
            u = in_slot[b]
            if u is not None and tick == start[b]:
                ss.open(b)
            live = u is not None and tick >= start[b] and ss.state[b] == "open" and not _sits(tick, b)
            cur.append(utts[u] if live else None)
        x, nv = _chunk_of(cur, pos, C)
        fin = [cur[b] is not None and pos[b] + C >= cur[b].shape[0] for b in range(3)]
        got = ss.push(x, nv, fin)
        log.append((got, [ss.status(b) for b in range(3)], ss.endpoints()))
        for b in range(3):
            pos[b] += nv[b]
            if fin[b]:
                u = in_slot[b]
                if kl is not None:
                    enc, lens = ss.encoder_output([b])
                    with model.given_encoder_output(enc):
                        want = model.spot_keywords(Pack(wave=torch.zeros(1, enc.shape[1], 1, dtype=enc.dtype, device=DEV), wave_len=lens), kl)[0]
                    res[u] = (ss.keyword_hits(b), ss.keywords_dropped(b), want)
                ss.finish(b, timestamps=False)
                if kl is not None:
                    assert ss.keyword_hits(b) == res[u][0]      # the list stays until the slot is opened again
                in_slot[b], pos[b], start[b] = (3, 0, tick + 1) if u == 2 else (None, 0, 0)
        tick += 1
        assert tick < 200
    return log, res


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["greedy", "timed", "prefix_beam"])
def test_sessions_with_keywords(mode, dtype):
    from tests.test_sessions_gpu import _feats, _model
    C = 8
    model = _model(dtype, -1)
    utts = _feats([6 * C, 5 * C - 3, C - 2, 3 * C], dtype, 3)      # one ends inside its first chunk, one on a chunk boundary
    kl = _session_keywords(model, utts)
    kw = dict(search="prefix_beam", beam_size=4, frame_topk=6) if mode == "prefix_beam" else dict(search="greedy", timed=mode == "timed")
    log, res = _drive(model, utts, C, kl, **kw)
    plain, _ = _drive(model, utts, C, None, **kw)
    assert log == plain      # the ids, the counters and the endpoints of the same sessions without keywords
    assert sorted(res) == [0, 1, 2, 3]
    for u, (hits, dropped, want) in res.items():
        assert hits == want["hits"] and dropped == want["dropped"] == 0, u
    assert sum(len(r[0]) for r in res.values()) > 8
    assert any(h["end_frame"] - h["start_frame"] >= 1 for r in res.values() for h in r[0])


def test_stream_with_keywords_and_the_refusals():
    from asr_chinese_e2e_amd.Utils import Pack
    from tests.test_sessions_gpu import _chunk_of, _feats, _model
    C = 8
    model = _model("fp32", -1)
    utts = _feats([4 * C, 2 * C + 3], "fp32", 5)
    kl = _session_keywords(model, utts)
    st = model.stream(2, keywords=kl)
    for c0 in range(0, 5 * C, C):      # the fifth push brings no frame: it only closes utterance 0
        st.push(*_chunk_of(utts, [c0, c0], C))
    enc, lens = st.encoder_output()
    with model.given_encoder_output(enc):
        want = model.spot_keywords(Pack(wave=torch.zeros(2, enc.shape[1], 1, device=DEV), wave_len=lens), kl)
    assert st.keyword_hits() == [w["hits"] for w in want] and sum(len(w["hits"]) for w in want) > 2
    with pytest.raises(ValueError, match="keyword_hits"):
        model.stream(2).keyword_hits()
    with pytest.raises(ValueError, match="blank_skip"):
        model.sessions(2, search="prefix_beam", blank_skip=0.98, keywords=kl)
    with pytest.raises(ValueError, match="KeywordList"):
        model.sessions(2, keywords=[[1, 2]])


# ------------------------------------------------------------------------------------------------ long recordings
def test_spot_long_equals_the_segments_shifted():
    from asr_chinese_e2e_amd.Utils import Pack
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.keywords import KeywordList
    from tests import vad_cases as C
    from tests.test_align_long_gpu import _model
    model = _model("fp32")
    parser = AudioParser(n_mels=80, lfr_m=4, lfr_n=3, device=DEV, frontend="kaldi")
    x = C.long_case()
    wav = torch.from_numpy(np.stack([x, np.zeros_like(x)])).to(DEV)      # the recording, and one without speech
    tr = model.transcribe_long(parser, wav[:1], [len(x)], batch_size=2, beam_size=3, joint="ctc_rescore", **C.LONG_OPTS)[0]
    assert len(tr["segments"]) == C.LONG_SEGMENTS >= 3      # at least two pauses
    ids = [i for i in tr["ids"] if i != 0]
    words = [ids[i:i + m] for m in (1, 2) for i in range(0, len(ids) - m + 1, 2)][:30] + [[4, 4]]
    kl = KeywordList(words, threshold=0.3, vocab_size=30, hits_per_keyword=16, max_hits=256)
    got, silent = model.spot_long(parser, wav, [len(x), len(x)], kl, batch_size=2, **C.LONG_OPTS)
    assert silent["hits"] == [] and silent["dropped"] == 0 and silent["segments"] == []
    assert got["segments"] == [(s["start_s"], s["end_s"]) for s in tr["segments"]] and got["duration_s"] == C.LONG_SECONDS
    want = []
    for i, s in enumerate(tr["segments"]):
        a, b = s["start_sample"], int(round(s["end_s"] * 16000))
        feats, flen = parser.parse_batch(torch.from_numpy(x[None, a:b].copy()).to(DEV), _i32([b - a]))
        for h in model.spot_keywords(Pack(wave=feats, wave_len=flen), kl)[0]["hits"]:
            want.append(dict(h, start_s=h["start_s"] + a / 16000.0, end_s=h["end_s"] + a / 16000.0, segment=i))
    assert len(want) > 4 and len({h["segment"] for h in want}) >= 2
    # a segment's bits do not depend on its batch (batch_size 2 against 1), so the lists are equal, not close
    assert got["hits"] == want
