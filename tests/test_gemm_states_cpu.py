"""What tests/test_gemm_states_gpu.py rests on, checked without a GPU: the restated planners of tests/gemm_cases.py cover the reduction
range exactly and agree with the library's own plan, the case tables reach every state they were written for (so an edit of a table
cannot silently lose one), every case keeps the bound that makes its result exact, and the checker sees each kind of defect."""
import pytest
import torch

from tests import gemm_cases as G

CUS = [8, 16, G.DEVICE_CUS]


def _tile_counts():
    return sorted({G.ceil_div(N, 128) * G.ceil_div(K, 128) for _, N, K in G.tn_shapes()})


def _assert_partition(ranges, M, what):
    assert ranges[0][0] == 0 and ranges[-1][1] == M, f"{what}: {ranges[0]} .. {ranges[-1]} does not span [0, {M})"
    for (b0, e0), (b1, e1) in zip(ranges, ranges[1:]):
        assert b1 == e0, f"{what}: split [{b1}, {e1}) does not start where [{b0}, {e0}) ended"
    assert all(e > b for b, e in ranges), f"{what}: empty split in {ranges}"


def test_splits_partition_the_reduction_range():
    """Every M in 1 .. 20000 (stride 13 above 5000), tile counts of the tables, 8 / 16 / 256 CUs: the splits [mbeg, mend) of the single
    launch, of the multi launch and of the grouped kernel start at 0, follow each other without gap or overlap, end at M; none is empty."""
    ms = list(range(1, 5001)) + list(range(5001, 20001, 13)) + [20000]
    reasons = set()
    for cus in CUS:
        for tiles in _tile_counts():
            N, K = 128 * tiles, 128
            for M in ms:
                st = G.tn_state(M, N, K, cus)
                reasons.add(st.why)
                _assert_partition(st.ranges, M, f"tn_plan M={M} tiles={tiles} cus={cus}")
                assert len(st.ranges) == st.nsplit
                assert all((e - b) % G.TM == 0 for b, e in st.ranges[:-1]), "only the last split may end inside a stage"
        for group in G.TN_GROUPS.values():
            for M in [m for m in ms if m % 7 == 0 or m < 600]:
                shapes = [(M, N, K) for _, N, K, _ in group]
                multi = G.tn_multi_plan(shapes, cus)
                if multi is not None:
                    _assert_partition(multi[4], M, f"tn_multi M={M} cus={cus}")
                    assert all((e - b) % G.TM == 0 for b, e in multi[4][:-1])
                shapes = [(max(1, M * (i + 1) // len(group)), N, K) for i, (_, N, K, _) in enumerate(group)]
                for (m, _, _), ranges in zip(shapes, G.tn_grouped_plan(shapes, cus)[1]):
                    _assert_partition(ranges, m, f"grouped M={m} cus={cus}")
    # the conditions of tn_stagger that these sizes reach; its third (the last split would start behind M) is met by none of them, so the
    # case tables cannot hold it
    assert reasons == {"fewer than 3 splits", "staggered", "declined: skew below one stage", "declined: first split below 4 stages"}, reasons


@pytest.fixture
def cu_limit():
    from asr_chinese_e2e_amd import kernels

    def set_limit(n):
        kernels.set_cu_limit(n)
    try:
        yield set_limit
    finally:
        kernels.set_cu_limit(0)


def test_restatement_agrees_with_the_library(deterministic_mode, cu_limit):
    """asr_gemm_tn_workspace_bytes is nsplit * (N * K + N) * 4 in deterministic mode: the library's nsplit equals the restatement's over a
    grid of (M, N, K, cu_limit) - the case tables included.  (Without a device cu_count() falls back to 256 CUs.)"""
    from asr_chinese_e2e_amd import kernels
    shapes = set(G.tn_shapes())
    for M in (1, 64, 255, 256, 257, 400, 513, 577, 1000, 1281, 1540, 2241, 4100, 8197, 16000, 20000):
        for N, K in ((8, 8), (128, 128), (136, 72), (256, 128), (384, 128), (512, 512), (1160, 1032), (1536, 512), (4232, 512)):
            shapes.add((M, N, K))
    for limit in (0, 1, 8, 12, 16, 64, 255, 256, 300):
        cu_limit(limit)
        cus = G.cu_count(limit)
        for M, N, K in sorted(shapes):
            need = kernels.lib.asr_gemm_tn_workspace_bytes(M, N, K)
            assert need % ((N * K + N) * 4) == 0
            assert need // ((N * K + N) * 4) == G.tn_plan(M, N, K, cus)[2], f"nsplit of {M}x{N}x{K} under cu_limit {limit}"


# ------------------------------------------------------------------------------------------------------------------ state coverage
def _nt_states():
    """state -> the first case of the tables that reaches it"""
    st = {}

    def reach(name, c):
        st.setdefault(name, f"{c.table} {c.M}x{c.N}x{c.K} limit {c.limit}")
    for c in G.nt_cases():
        ldc = G.nt_ldc(c)
        branch = G.nt_branch(c.M, c.N, c.K, ldc, c.act, c.bias, c.res is not None, c.c_off)
        if c.branch is not None:
            assert branch == c.branch, f"{c}: lands on {branch}"
        assert branch != "refused", c
        if branch == "all_in_one":
            ragged = c.K % 64 != 0
            for why, hit in (("K < 128", c.K < 128), ("ragged K with ReLU", ragged and c.act == G.ACT_RELU), ("ragged K with res", ragged and c.res is not None),
                             ("bias with res", c.bias and c.res is not None), ("C 8 bytes off", c.c_off % 16 == 8),
                             ("scalar tail of %d" % (c.N % 4), c.N % 4 != 0 and ldc % 8 != 0), ("ragged K with ReLU, no bias", ragged and c.act == G.ACT_RELU and not c.bias)):
                if hit:
                    reach(f"all-in-one: {why}", c)
            continue
        reach(f"branch {branch}", c)
        w = G.nt_walk(c.M, c.N, c.K, G.cu_count(c.limit))
        kind = "ragged" if c.K % 64 else "even"
        tail = {(0, False): "plain", (0, True): "bias", (1, False): "relu", (1, True): "relu+bias"}[(c.act, c.bias)] if c.res is None else \
            ("mask" if c.act == G.ACT_RELU_MASK else "res in place" if c.res == "inplace" else "res")
        for mt in set(w.my_tiles):
            assert mt > 0
            reach(f"ring {kind} nk={w.nk} my_tiles={mt} total%3={mt * w.nk % 3} [{'bias' if tail == 'bias' else 'tails'}]", c)
            if mt > 1:
                reach(f"tail {tail} with my_tiles={mt} nk={w.nk}", c)
        if w.ntiles < 8:
            reach("XCD shares of zero (fewer than 8 tiles)", c)
        if w.trem and w.ntiles > 8:
            reach("ntiles % 8 != 0", c)
        if w.grid in (8, 16):
            reach(f"grid of exactly {w.grid}", c)
        if w.grid % 8 and w.grid > 8:
            reach("grid no multiple of 8 (nb_x differs between XCDs)", c)
        if c.limit == 8 and w.ntiles == 20:
            assert w.shares == [3, 3, 3, 3, 2, 2, 2, 2]
            reach("XCD shares 3,3,3,3,2,2,2,2", c)
        if w.full_tiles:
            reach("full tiles (unpredicated store tail)", c)
        if w.partial_tiles:
            reach("partial tiles (predicated store tail)", c)
        if w.full_tiles and w.partial_tiles and max(w.my_tiles) > 1:
            reach("full and partial tiles in one walk", c)
        if c.table == "edge":
            reach(f"edge M={c.M}", c)
            reach(f"edge N={c.N} ({tail})", c)
        if G.ceil_div(c.N, 128) > 1 and max(w.my_tiles) > 1:
            reach("two tile columns, several tiles per workgroup", c)
    return st


def _nt_required():
    need = ["branch persistent:mask", "branch persistent:res", "branch persistent:ragged", "branch persistent:plain", "branch persistent:relu",
            "all-in-one: K < 128", "all-in-one: ragged K with ReLU", "all-in-one: ragged K with ReLU, no bias", "all-in-one: ragged K with res",
            "all-in-one: bias with res", "all-in-one: C 8 bytes off",
            "all-in-one: scalar tail of 1", "all-in-one: scalar tail of 2", "all-in-one: scalar tail of 3",
            "XCD shares of zero (fewer than 8 tiles)", "ntiles % 8 != 0", "grid of exactly 8", "grid of exactly 16", "grid no multiple of 8 (nb_x differs between XCDs)",
            "XCD shares 3,3,3,3,2,2,2,2", "full tiles (unpredicated store tail)", "partial tiles (predicated store tail)", "full and partial tiles in one walk",
            "two tile columns, several tiles per workgroup"]
    for nk in (2, 3, 4, 5, 7):      # every ring phase at a tile boundary: one, two and three tiles per workgroup
        need += [f"ring even nk={nk} my_tiles={mt} total%3={mt * nk % 3} [bias]" for mt in (1, 2, 3)]
    for nk in (2, 3, 4):
        need += [f"ring ragged nk={nk} my_tiles={mt} total%3={mt * nk % 3} [bias]" for mt in (1, 2, 3)]
        need += [f"ring even nk={nk} my_tiles={mt} total%3={mt * nk % 3} [tails]" for mt in (1, 2, 3)]
        need += [f"tail {t} with my_tiles={mt} nk={nk}" for t in ("relu+bias", "mask", "res", "res in place") for mt in (2, 3)]
    need += [f"edge M={M}" for M in (1, 8, 255, 256, 257)]
    need += [f"edge N={N} ({t})" for N in (8, 120, 128, 136, 264) for t in ("bias", "relu+bias", "mask", "res", "res in place")]
    return need


def _tn_states():
    st = {}

    def reach(name, shape, limit):
        st.setdefault(name, f"{shape[0]}x{shape[1]}x{shape[2]} limit {limit}")
    for limit in G.TN_LIMITS:
        where = "whole device" if limit == 0 else f"cu_limit {limit}"
        cus = G.cu_count(limit)
        for s in G.tn_shapes():
            M, N, K = s
            t = G.tn_state(M, N, K, cus)
            if t.nsplit == 1:
                nsteps = G.ceil_div(M, G.TM)
                reach(f"one split: {nsteps} stage{'s' if nsteps > 1 else ''}, {'ragged' if M % G.TM else 'whole'}, ring {t.ring}", s, limit)
                if s in G.TN_TAIL_SHAPES:
                    reach(f"tails N={N} K={K}", s, limit)
                continue
            last = t.ranges[-1][1] - t.ranges[-1][0]
            if t.nsplit == 2:
                reach(f"two splits [{where}]", s, limit)
            if t.nsplit >= 3 and t.skew > 0:
                reach(f"three or more splits, skew > 0 [{where}]", s, limit)
            if t.nsplit >= 3 and t.skew == 0:
                reach(f"three or more splits, {t.why} [{where}]", s, limit)
            reach(f"ring {t.ring}, several splits [{where}]", s, limit)
            if last < G.TM:
                reach(f"last split shorter than one stage [{where}]", s, limit)
            if M % G.TM:
                reach(f"several splits, M no multiple of 64 [{where}]", s, limit)
        for name, group in G.TN_GROUPS.items():
            shapes = [g[:3] for g in group]
            multi = G.tn_multi_plan(shapes, cus)
            if multi is None:
                R, ranges = G.tn_grouped_plan(shapes, cus)
                kinds = sorted({"several splits" if len(r) > 1 else "one split" for r in ranges})
                reach(f"grouped kernel ({', '.join(kinds)}) [{where}]", (name, "R", R), limit)
            else:
                reach(f"multi launch, {multi[3]} [{where}]", (name, multi[0], "splits"), limit)
    return st


def _tn_required():
    need = [f"one split: {n} stage{'s' if n > 1 else ''}, {r}, ring 3" for n, r in ((1, "ragged"), (1, "whole"), (2, "ragged"), (2, "whole"), (3, "ragged"), (3, "whole"),
                                                                                  (4, "ragged"), (4, "whole"))]
    need += [f"one split: {n} stage{'s' if n > 1 else ''}, {r}, ring 2" for n, r in ((1, "ragged"), (1, "whole"), (3, "ragged"), (4, "ragged"))]      # cu_limit 8, three tiles
    for where in ("whole device", "cu_limit 8"):
        need += [f"{s} [{where}]" for s in ("two splits", "three or more splits, skew > 0", "three or more splits, declined: skew below one stage",
                                           "three or more splits, declined: first split below 4 stages", "ring 2, several splits", "ring 3, several splits",
                                           "last split shorter than one stage", "several splits, M no multiple of 64")]
    need += [f"tails N={N} K={K}" for N in (8, 136) for K in (8, 72, 136)]
    need += ["multi launch, declined: skew below one stage [whole device]", "multi launch, staggered [cu_limit 8]",
             "grouped kernel (one split, several splits) [whole device]", "grouped kernel (one split, several splits) [cu_limit 8]",
             "grouped kernel (several splits) [cu_limit 8]"]
    return need


def test_case_tables_reach_every_state():
    """Every state the tables were written for is reached by at least one case, and every ladder case lands on the branch its comment
    names.  `pytest -s` prints the list (state: first case that reaches it)."""
    nt, tn = _nt_states(), _tn_states()
    for title, st in (("NT", nt), ("TN", tn)):
        print(f"\n{title} states ({len(st)})")
        for name in sorted(st):
            print(f"  {name}: {st[name]}")
    missing = [n for n in _nt_required() if n not in nt] + [n for n in _tn_required() if n not in tn]
    assert not missing, f"no case reaches: {missing}"
    # the two candidates worked out by hand for 8 CUs
    assert G.tn_state(1600, 256, 128, 8)[:4] == (3, 4, 320, 64)
    assert G.tn_state(1400, 384, 128, 8).ring == 2


def test_operands_cover_every_k_chunk():
    """Between them the rows of A hit every 8-element chunk of every k-step with a non-zero that meets a non-zero of W"""
    for K in sorted({c.K for c in G.nt_cases()}):
        for M in (8, 219):
            hit = (G.nt_a(M, K) != 0).view(M, K // 8, 8).any(2).any(0)
            assert bool(hit.all()), f"K={K} M={M}: chunks {(~hit).nonzero().flatten().tolist()} never hit"
        w = G.nt_w(G.NT_MAX_N, K)
        assert int(w.min()) == -2 and int(w.max()) == 2 and not torch.equal(w[:64, :64], w[:64, :64].t())
        assert len({tuple(r) for r in w.tolist()}) == G.NT_MAX_N and len({tuple(r) for r in w.t().tolist()}) == K, "rows or columns of W repeat"
        assert int((G.nt_a(300, K) != 0).sum(1).max()) <= G.NT_NNZ


# ------------------------------------------------------------------------------------------------------------------ bounds
@pytest.fixture(scope="module")
def nt_data():
    return G.NtData("cpu")


@pytest.fixture(scope="module")
def tn_data():
    return G.TnData("cpu")


def test_every_case_keeps_its_exactness_bound(nt_data, tn_data):
    """NT: |product|, |product + bias|, |.. + res| <= 256 (nt_reference asserts each); TN: the sum of magnitudes, which bounds every
    partial sum in any order, stays below 2^24 with the start values (tn_reference asserts it)."""
    seen = set()
    for c in G.nt_cases():
        key = (c.M, c.N, c.K, c.act, c.bias, c.res is not None)
        if key in seen:
            continue
        seen.add(key)
        ref = nt_data.reference(c)
        assert ref.dtype == torch.int64 and int(ref.abs().max()) <= G.NT_BOUND
        assert torch.equal(ref.bfloat16().to(torch.int64), ref)
    for M, N, K in G.tn_shapes() + [g[:3] for grp in G.TN_GROUPS.values() for g in grp]:
        for acc in (True, False):
            dw, db = tn_data.reference(M, N, K, acc)
            assert int(dw.abs().max()) < G.TN_BOUND and int(db.abs().max()) < G.TN_BOUND
            assert torch.equal(dw.float().to(torch.int64), dw)
    assert int(tn_data.dy.abs().max()) == 4 and int(tn_data.x.abs().max()) == 4


# ------------------------------------------------------------------------------------------------------------------ the checker
def _expect_failure(buf, init, ref, rows, cols, off=0):
    with pytest.raises(AssertionError):
        G.check_exact(buf, init, ref, rows, cols, off, what="defect")


def test_checker_sees_each_defect_nt(nt_data):
    """An NT case (ring table, three tiles, K = 192): the exact result passes; one reduction element (a k "row" of the product) dropped,
    one counted twice, one 8-column chunk of one k-step dropped, one output off by one, one sentinel overwritten - each fails."""
    c = next(c for c in G.nt_ring_cases() if c.K == 192 and c.M == 256 * 3 - 37 and c.bias)
    a, w, bias, res, out, (cbuf, init, off) = nt_data.operands(c)
    ref = nt_data.reference(c)
    ai, wi = G.nt_a(c.M, c.K), G.nt_w(c.N, c.K)

    def result(a_used):
        return G.nt_reference(G.exact_matmul_nt(a_used, wi), c.act, nt_data.bias[:c.N], None)
    assert torch.equal(result(ai), ref)
    good = init.clone()
    good[:c.M, off:off + c.N] = ref.bfloat16()
    G.check_exact(good, init, ref, c.M, c.N, off)
    k = 77
    assert bool((ai[:, k] != 0).any())
    dropped = ai.clone()
    dropped[:, k] = 0                                        # reduction index k never added
    twice = ai.clone()
    twice[:, k] *= 2                                         # reduction index k added twice
    chunk = ai.clone()
    chunk[:, 128 + 24:128 + 32] = 0                          # chunk 3 of k-step 2
    for a_bad in (dropped, twice, chunk):
        bad = init.clone()
        bad[:c.M, off:off + c.N] = result(a_bad).bfloat16()
        _expect_failure(bad, init, ref, c.M, c.N, off)
    one_row = good.clone()                                   # a single output row that lost one product: the smallest trace a lost row can leave
    m = int((ai[:, k] != 0).nonzero()[0])
    n = int((wi[:, k] != 0).nonzero()[0])
    one_row[m, off + n] = float(ref[m, n] - ai[m, k] * wi[n, k])
    _expect_failure(one_row, init, ref, c.M, c.N, off)
    off_by_one = good.clone()
    off_by_one[c.M - 1, off + c.N - 1] += 1
    _expect_failure(off_by_one, init, ref, c.M, c.N, off)
    for r, col in ((c.M, 0), (c.M - 1, off + c.N), (0, off + c.N + G.PAD - 1)):
        spoiled = good.clone()
        spoiled[r, col] = 0.0
        _expect_failure(spoiled, init, ref, c.M, c.N, off)
    neg_zero = good.clone()                                  # bit patterns, not values: -0.0 is not +0.0
    r0, c0 = [int(v) for v in (ref == 0).nonzero()[0]]
    neg_zero[r0, off + c0] = -0.0
    _expect_failure(neg_zero, init, ref, c.M, c.N, off)


def test_checker_sees_each_defect_tn(tn_data):
    """A TN case (1600 x 256 x 128: four staggered splits under 8 CUs): one reduction row dropped at a split boundary, one counted
    twice, one 8-column chunk of one stage dropped, one element off by one, one sentinel overwritten - each fails; so does a lost dbias row."""
    M, N, K = 1600, 256, 128
    boundary = G.tn_state(M, N, K, 8).ranges[1][0]
    assert boundary == 320
    dy, x, dw, dbias, wbuf, winit, bbuf, binit = tn_data.operands(M, N, K, True, True)
    ref_w, ref_b = tn_data.reference(M, N, K, True)
    yi, xi = G.tn_dy(M, N), G.tn_x(M, K)
    assert torch.equal(G.tn_reference(yi, xi, tn_data.dw0[:N, :K], tn_data.db0[:N])[0], ref_w)
    good = winit.clone()
    good[:N, :K] = ref_w.float()
    G.check_exact(good, winit, ref_w, N, K)
    good_b = binit.clone()
    good_b[0, :N] = ref_b.float()
    G.check_exact(good_b, binit, ref_b.unsqueeze(0), 1, N)
    row = yi[boundary].unsqueeze(1) * xi[boundary].unsqueeze(0)
    assert int(row.abs().max()) > 0
    chunk = yi[boundary:boundary + 64].t() @ torch.cat([torch.zeros(64, 8, dtype=torch.int64), xi[boundary:boundary + 64, 8:16], torch.zeros(64, K - 16, dtype=torch.int64)], 1)
    assert int(chunk.abs().max()) > 0
    for delta in (-row, row, -chunk):
        bad = good.clone()
        bad[:N, :K] = (ref_w + delta).float()
        _expect_failure(bad, winit, ref_w, N, K)
    bad = good.clone()
    bad[N - 1, K - 1] += 1
    _expect_failure(bad, winit, ref_w, N, K)
    for r, col in ((N, 0), (0, K), (N + 1, K + G.PAD - 1)):
        bad = good.clone()
        bad[r, col] = 0.0
        _expect_failure(bad, winit, ref_w, N, K)
    bad_b = good_b.clone()
    bad_b[0, :N] = (ref_b - yi[boundary]).float()
    if int(yi[boundary].abs().max()) > 0:
        _expect_failure(bad_b, binit, ref_b.unsqueeze(0), 1, N)
    bad_b = good_b.clone()
    bad_b[0, N] = 0.0
    _expect_failure(bad_b, binit, ref_b.unsqueeze(0), 1, N)
