"""Weight averaging without a GPU: the definition of the exponential moving average (tests/ema_ref.py) against exact rational arithmetic,
checkpoint averaging (asr_chinese_e2e_amd/averaging.py) against an exact mean, checkpoint selection on a synthetic experiment directory, the
two new entry points of the C ABI and every refusal their launchers make before a launch."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import ema_ref as E


# ------------------------------------------------------------------------------------------------ exact rounding, for the restatements
def round_fraction(x, p, emin, emax):
    """The binary floating-point number with p significand bits and exponent range [emin, emax] nearest to the Fraction x (ties to even),
    as a Fraction; subnormals included.  Values that would overflow are not expected here."""
    if x == 0:
        return Fraction(0)
    sign = -1 if x < 0 else 1
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # floor(log2 a) is e or e - 1
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, emin) - p + 1)                      # spacing of the format at a
    k = a / q
    n = k.numerator // k.denominator
    r = k - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    out = n * q
    assert out < Fraction(2) ** (emax + 1)
    return sign * out


def f32(x):
    return round_fraction(x, 24, -126, 127)


def f64(x):
    return round_fraction(x, 53, -1022, 1023)


def bf16(x):
    return round_fraction(x, 8, -126, 127)


def ema_exact(e, p, decay, step, warmup):
    """The definition in Fractions, every rounding explicit."""
    d = Fraction(float(np.float32(decay)))
    if warmup:
        w = f64(Fraction(1 + step) / Fraction(10 + step))          # 1.0 + s and 10.0 + s are exact in float64
        d = min(d, w)
    omd = f32(f64(1 - d))                                          # 1.0 - d in float64, then one rounding to float32
    t = f32(Fraction(float(p)) - Fraction(float(e)))
    u = f32(omd * t)
    return f32(Fraction(float(e)) + u)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the definition
def test_round_fraction_is_numpy_rounding():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(100) * 10.0 ** rng.integers(-30, 30, 100), [1e-45, 3e-39, 1.0000000596046448, 0.1]])
    for x in xs:
        assert float(f32(Fraction(float(x)))) == float(np.float32(x))


@pytest.mark.parametrize("warmup", [True, False])
def test_ema_ref_equals_the_rational_restatement(warmup):
    rng = np.random.default_rng(1)
    n = 300
    e = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    p = (e + rng.standard_normal(n).astype(np.float32) * 10.0 ** rng.integers(-9, 1, n)).astype(np.float32)
    e[:5] = [0.0, 1e-40, -1e-40, 1.0, -3.5]                        # zero, subnormals, and p far from e
    p[:5] = [1e-42, -1e-40, 0.0, 1.0 + 2.0 ** -23, 1e8]
    for decay, step in ((0.999, 1), (0.999, 50), (0.9, 3), (0.5, 1000000), (0.9999, 8981)):
        got = E.ema_update(e, p, decay, step, warmup)
        assert got.dtype == np.float32
        want = np.array([float(ema_exact(e[i], p[i], decay, step, warmup)) for i in range(n)], dtype=np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (decay, step)


def test_warmup_coefficients_and_the_switch_to_decay():
    for s in (1, 2, 10, 1000, 10 ** 6):
        w = float(f64(Fraction(1 + s, 10 + s)))
        assert E.decay_at(0.999, s, True) == min(float(np.float32(0.999)), w)
        assert E.decay_at(0.999, s, False) == float(np.float32(0.999))
        assert float(E.one_minus_decay(0.999, s, True)) == float(np.float32(1.0 - E.decay_at(0.999, s, True)))
    assert E.decay_at(0.999, 1) == 2.0 / 11.0 and E.decay_at(0.999, 2) == 0.25 and E.decay_at(0.999, 10) == 0.55
    assert E.decay_at(0.999, 1000) == 1001.0 / 1010.0
    assert E.decay_at(0.999, 10 ** 6) == float(np.float32(0.999))
    # the switch to `decay`: the first step whose (1 + s) / (10 + s) exceeds 0.999.  (1 + s) / (10 + s) = 1 - 9 / (10 + s) > 0.999 <=>
    # 10 + s > 9000 <=> s >= 8991; the float32 nearest to 0.999 is 0.99900001287..., for which 10 + s > 9000.116 gives the same step
    d32 = float(np.float32(0.999))
    first = next(s for s in range(1, 20000) if Fraction(1 + s, 10 + s) > Fraction(d32))
    assert first == 8991 == next(s for s in range(1, 20000) if Fraction(1 + s, 10 + s) > Fraction(999, 1000))
    assert E.decay_at(0.999, first - 1) == 8991.0 / 9000.0 < d32 and E.decay_at(0.999, first) == d32 and E.decay_at(0.999, first + 1) == d32
    # without the warm-up an average read after 1000 steps still holds 0.999^1000 = 37 % of its initial value
    assert abs(0.999 ** 1000 - 0.3677) < 1e-4


def test_fixed_point_and_fold():
    rng = np.random.default_rng(2)
    p = (rng.standard_normal(500) * 10.0 ** rng.integers(-8, 8, 500)).astype(np.float32)
    for warmup in (True, False):
        for step in (1, 7, 100000):
            assert np.array_equal(_bits(E.ema_update(p, p, 0.999, step, warmup)), _bits(p))      # p == e is an exact fixed point
    ps = [p + np.float32(0.01 * k) for k in range(1, 4)]
    folded = E.ema_fold(p, ps, 0.9, first_step=5)
    e = p
    for k, q in enumerate(ps):
        e = E.ema_update(e, q, 0.9, 5 + k)
    assert np.array_equal(_bits(folded), _bits(e))


# ------------------------------------------------------------------------------------------------ checkpoint averaging
def _exact_mean(tensors, weights, dtype):
    """Per element (the definition in Fractions, the exactly rounded exact mean - slack, ... + slack).  The definition: float64(w_i) *
    float64(x_i) accumulated in the order given, divided by the float64 sum of the weights, rounded once to the dtype - every float64
    rounding explicit.  slack bounds what those float64 roundings can add to the exact mean: N products, N - 1 sums, the sum of the
    weights and one division, each within 2^-53 relative of its exact value."""
    rnd = {torch.float32: f32, torch.bfloat16: bf16}[dtype]
    flat = [t.double().reshape(-1).tolist() for t in tensors]
    ws = [Fraction(float(w)) for w in weights]
    tot = sum(ws)
    out = []
    for j in range(len(flat[0])):
        terms = [w * Fraction(x[j]) for w, x in zip(ws, flat)]
        acc = f64(terms[0])
        for t in terms[1:]:
            acc = f64(acc + f64(t))
        by_definition = rnd(f64(acc / f64(tot)))
        mean = sum(terms) / tot
        slack = (2 * len(terms) + 2) * Fraction(1, 2 ** 53) * sum(abs(t) for t in terms) / tot
        out.append((by_definition, rnd(mean - slack), rnd(mean + slack)))
    return out


def _check_mean(got, tensors, weights):
    """Bit for bit the definition, which is the exactly rounded exact mean wherever that mean is not within float64 round-off of a
    rounding boundary of the dtype (the mean of two float32 numbers often IS such a boundary: then either neighbour is a correct rounding
    of a value within the slack, and the definition picks one)."""
    vals = got.double().reshape(-1).tolist()
    for v, (d, lo, hi) in zip(vals, _exact_mean(tensors, weights, got.dtype)):
        assert Fraction(v) == d
        assert lo <= d <= hi


def _dicts(n, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    pe = torch.arange(12, dtype=torch.float32).reshape(1, 3, 4)
    return [{"w": (torch.randn(5, 7, generator=g) * 3).to(dtype), "b": torch.randn(7, generator=g).to(dtype), "pe": pe.clone(),
             "steps": torch.tensor([3], dtype=torch.int64)} for _ in range(n)]


@pytest.mark.parametrize("n", [1, 2, 3, 30])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_average_state_dicts_is_the_exact_mean(n, dtype):
    from asr_chinese_e2e_amd.averaging import average_state_dicts
    ds = _dicts(n, seed=n, dtype=dtype)
    avg = average_state_dicts(ds)
    assert list(avg.keys()) == list(ds[0].keys())
    for k in ("w", "b"):
        assert avg[k].dtype == dtype and avg[k].shape == ds[0][k].shape
        _check_mean(avg[k], [d[k] for d in ds], [1] * n)
    assert torch.equal(avg["pe"], ds[0]["pe"]) and avg["pe"] is not ds[0]["pe"]
    assert torch.equal(avg["steps"], ds[0]["steps"])
    if n == 1:
        assert all(torch.equal(avg[k], ds[0][k]) for k in avg)


def test_average_state_dicts_weights_order_and_identical_inputs(tmp_path):
    from asr_chinese_e2e_amd.averaging import average_state_dicts
    ds = _dicts(3, seed=9)
    w = [0.5, 2.0, 0.25]
    avg = average_state_dicts(ds, weights=w)
    for k in ("w", "b"):
        _check_mean(avg[k], [d[k] for d in ds], w)
    # a weight of zero leaves a checkpoint out
    a = average_state_dicts(ds, weights=[1, 0, 1])
    b = average_state_dicts([ds[0], ds[2]])
    assert all(torch.equal(a[k], b[k]) for k in a)
    # order of the inputs: the same exact mean either way (float64 accumulation cannot move a float32 rounding except on a boundary)
    r = average_state_dicts(ds[::-1], weights=w[::-1])
    for k in ("w", "b"):
        _check_mean(r[k], [d[k] for d in ds], w)
    # identical inputs come back bit for bit, whatever N and the weights
    same = average_state_dicts([ds[0]] * 7, weights=[0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7])
    for k in same:
        assert torch.equal(same[k].view(torch.int32) if same[k].dtype == torch.float32 else same[k], ds[0][k].view(torch.int32)
                           if ds[0][k].dtype == torch.float32 else ds[0][k]), k
    # paths are loaded
    paths = []
    for i, d in enumerate(ds):
        paths.append(str(tmp_path / f"e0_s{i}.model"))
        torch.save(d, paths[-1])
    from_files = average_state_dicts(paths, weights=w)
    assert all(torch.equal(from_files[k], avg[k]) for k in avg)


def test_average_state_dicts_refusals(tmp_path):
    from asr_chinese_e2e_amd.averaging import average_state_dicts
    ds = _dicts(2, seed=4)
    with pytest.raises(ValueError, match="empty"):
        average_state_dicts([])
    other = dict(ds[1])
    other["extra"] = torch.zeros(1)
    with pytest.raises(KeyError, match="extra"):
        average_state_dicts([ds[0], other])
    less = {k: v for k, v in ds[1].items() if k != "b"}
    with pytest.raises(KeyError, match="'b'"):
        average_state_dicts([ds[0], less])
    shape = dict(ds[1], w=torch.zeros(5, 8))
    with pytest.raises(ValueError, match="'w' has shape"):
        average_state_dicts([ds[0], shape])
    dt = dict(ds[1], w=ds[1]["w"].bfloat16())
    with pytest.raises(ValueError, match="'w' has dtype"):
        average_state_dicts([ds[0], dt])
    for bad in (float("nan"), float("inf")):
        nf = dict(ds[1], b=ds[1]["b"].clone())
        nf["b"][3] = bad
        with pytest.raises(ValueError, match="'b' of checkpoint 1 holds non-finite"):
            average_state_dicts([ds[0], nf])
    ints = dict(ds[1], steps=torch.tensor([4], dtype=torch.int64))
    with pytest.raises(ValueError, match="'steps'"):
        average_state_dicts([ds[0], ints])
    with pytest.raises(ValueError, match="not negative"):
        average_state_dicts(ds, weights=[1, -1])
    with pytest.raises(ValueError, match="not negative"):
        average_state_dicts(ds, weights=[1, float("nan")])
    with pytest.raises(ValueError, match="all zero"):
        average_state_dicts(ds, weights=[0, 0])
    with pytest.raises(ValueError, match="1 weights for 2"):
        average_state_dicts(ds, weights=[1])
    with pytest.raises(FileNotFoundError, match="nowhere.model"):
        average_state_dicts([str(tmp_path / "nowhere.model")])


# ------------------------------------------------------------------------------------------------ checkpoint selection
def _experiment(root, steps, records, ema=()):
    os.makedirs(root, exist_ok=True)
    for s in steps:
        torch.save({"w": torch.full((2,), float(s))}, os.path.join(root, f"e{s // 100}_s{s}.model"))
        torch.save({}, os.path.join(root, f"e{s // 100}_s{s}.opt"))
    for s in ema:
        torch.save({"w": torch.full((2,), float(s) + 0.5)}, os.path.join(root, f"e{s // 100}_s{s}.ema.model"))
    with open(os.path.join(root, "scalars.jsonl"), "w") as f:
        for tag, step, value in records:
            f.write(json.dumps({"tag": tag, "value": value, "step": step}) + "\n")
    with open(os.path.join(root, "notes.model.txt"), "w") as f:      # not a checkpoint
        f.write("x")


def test_select_checkpoints(tmp_path):
    from asr_chinese_e2e_amd.averaging import average_state_dicts, select_checkpoints
    root = str(tmp_path / "exp")
    steps = [100, 200, 300, 400, 1000, 50]
    records = [("dev/loss", 100, 3.0), ("dev/loss", 200, 1.0), ("dev/loss", 300, 2.0), ("dev/loss", 400, 1.0), ("dev/loss", 1000, 5.0),
               ("dev/loss", 150, 0.1),                               # a record, but no checkpoint at that step
               ("dev/acc", 100, 0.5), ("dev/acc", 200, 0.9), ("dev/acc", 300, 0.9), ("dev/acc", 400, 0.1), ("dev/acc", 1000, 0.2), ("dev/acc", 50, 0.3),
               ("dev/ema/loss", 200, 0.5), ("dev/ema/loss", 300, 0.4), ("lr", 100, 1e-3)]
    _experiment(root, steps, records, ema=[200, 300])
    name = lambda ps: [os.path.basename(p) for p in ps]      # noqa: E731
    assert name(select_checkpoints(root, 3)) == ["e3_s300.model", "e4_s400.model", "e10_s1000.model"]      # by step, not by name
    assert name(select_checkpoints(root, 6, mode="last")) == ["e0_s50.model", "e1_s100.model", "e2_s200.model", "e3_s300.model", "e4_s400.model",
                                                              "e10_s1000.model"]
    rep = []
    # lowest dev/loss: 200 and 400 tie at 1.0 - the later step goes first; step 50 has no dev/loss record
    assert name(select_checkpoints(root, 1, mode="best", report=rep)) == ["e4_s400.model"]
    assert len(rep) == 1 and "e0_s50.model" in rep[0] and "step 50" in rep[0]
    assert name(select_checkpoints(root, 2, mode="best", report=[])) == ["e2_s200.model", "e4_s400.model"]
    assert name(select_checkpoints(root, 3, mode="best", metric="-dev/loss", report=[])) == ["e2_s200.model", "e3_s300.model", "e4_s400.model"]
    # '+': highest; 200 and 300 tie at 0.9 - the later first
    assert name(select_checkpoints(root, 1, mode="best", metric="+dev/acc", report=[])) == ["e3_s300.model"]
    assert name(select_checkpoints(root, 3, mode="best", metric="+dev/acc", report=[])) == ["e1_s100.model", "e2_s200.model", "e3_s300.model"]
    # the averages a run with ema_decay writes
    assert name(select_checkpoints(root, 2, which="ema")) == ["e2_s200.ema.model", "e3_s300.ema.model"]
    assert name(select_checkpoints(root, 1, mode="best", metric="dev/ema/loss", which="ema", report=[])) == ["e3_s300.ema.model"]
    avg = average_state_dicts(select_checkpoints(root, 2, which="ema"))
    assert avg["w"].tolist() == [250.5, 250.5]
    # too few
    with pytest.raises(ValueError, match="6 usable checkpoints"):
        select_checkpoints(root, 7)
    with pytest.raises(ValueError, match="5 usable checkpoints"):
        select_checkpoints(root, 6, mode="best", report=[])
    with pytest.raises(ValueError, match="2 usable"):
        select_checkpoints(root, 3, which="ema")
    with pytest.raises(ValueError, match="0 usable"):
        select_checkpoints(root, 1, mode="best", metric="dev/cer", report=[])
    with pytest.raises(ValueError, match="mode"):
        select_checkpoints(root, 1, mode="median")
    with pytest.raises(ValueError, match="which"):
        select_checkpoints(root, 1, which="opt")


def test_average_cli(tmp_path, capsys):
    import average
    root = str(tmp_path / "exp")
    _experiment(root, [100, 200, 300], [("dev/loss", 100, 1.0), ("dev/loss", 200, 3.0), ("dev/loss", 300, 2.0)])
    out = str(tmp_path / "avg.model")
    paths = average.main([f"--exp={root}", "--num=2", "--mode=best", "--metric=dev/loss", f"--out={out}"])
    assert [os.path.basename(p) for p in paths] == ["e1_s100.model", "e3_s300.model"]
    printed = capsys.readouterr().out
    assert "e1_s100.model" in printed and "e3_s300.model" in printed and "e2_s200.model" not in printed
    assert torch.load(out, weights_only=True)["w"].tolist() == [200.0, 200.0]
    with pytest.raises(SystemExit, match="3 usable"):
        average.main([f"--exp={root}", "--num=4", f"--out={out}"])
    with pytest.raises(SystemExit, match="--out"):
        average.main([f"--exp={root}"])


# ------------------------------------------------------------------------------------------------ configuration
def _tiny(**kw):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = Models.TransformerCTC
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=8, lfr_m=1, d_model=16, hidden_size=8, num_head=2, ff_size=16, layer_num=1, dropout=0.0, ctc_weight=1.0, dtype="fp32", **kw))
    return M(cfg, Vocab.synthetic(12))


def test_config_keys_and_their_refusals(tmp_path):
    from asr_chinese_e2e_amd import Models
    cfg = Models.TransformerOffical.get_default_config()()
    assert cfg.ema_decay == 0.0 and cfg.ema_warmup is True
    m = _tiny()
    assert m.ema_decay == 0.0 and m._flat.ema is None
    for call in (m.ema_state_dict, lambda: m.save_ema(str(tmp_path / "x")), lambda: m.load_ema(str(tmp_path / "x")), lambda: m.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay is 0"):
            call()
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), 0.99999999, "0.9", True):      # 0.99999999 is 1.0 as a float32
        with pytest.raises(ValueError, match="ema_decay"):
            _tiny(ema_decay=bad)
    m = _tiny(ema_decay=0.999, ema_warmup=False)
    assert m.ema_decay == 0.999 and m.ema_warmup is False
    # before the flat buffers exist the average is the parameters themselves, under the model's keys
    sd, avg = m.state_dict(), m.ema_state_dict()
    assert list(avg.keys()) == list(sd.keys()) and all(torch.equal(avg[k], sd[k]) for k in sd)
    m.save_ema(str(tmp_path / "a.ema.model"))
    short = {k: v for k, v in avg.items() if k != "ctc_lo.bias"}
    torch.save(short, str(tmp_path / "short.model"))
    with pytest.raises(KeyError, match="ctc_lo.bias"):
        m.load_ema(str(tmp_path / "short.model"))
    m.load_ema(str(tmp_path / "a.ema.model"))
    plain = _tiny()
    assert not plain.load_state_dict(torch.load(str(tmp_path / "a.ema.model"), weights_only=True), strict=True).missing_keys


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_and_abi_version():
    from asr_chinese_e2e_amd import _lib
    from ctypes import c_float, c_int, c_size_t, c_void_p
    assert _lib.lib.asr_abi_version() == 10 == _lib.ABI_VERSION
    P, I, F, Z = c_void_p, c_int, c_float, c_size_t
    assert _lib.SIGNATURES["asr_adam_ema_step"] == (I, _lib.SIGNATURES["asr_adam_step"][1][:-1] + [P, F, I, P])
    assert _lib.SIGNATURES["asr_ema_update"] == (I, [P, P, Z, F, I, F, P])
    assert hasattr(_lib.lib, "asr_adam_ema_step") and hasattr(_lib.lib, "asr_ema_update")
    assert hasattr(_lib.fast, "asr_adam_ema_step") and hasattr(_lib.fast, "asr_ema_update")


A = 0x7f0000001000      # a 16-byte aligned address nothing reads: every call below is refused before a launch


@pytest.mark.parametrize("route", ["ctypes", "fast"])
def test_launcher_refusals(route):
    from asr_chinese_e2e_amd import _lib
    L = _lib.lib if route == "ctypes" else _lib.fast
    none = None if route == "ctypes" else 0
    nan, inf = float("nan"), float("inf")

    def adam(p=A, g=A + 64, m=A + 128, v=A + 192, lp=none, n=8, hyper=A + 256, sumsq=A + 320, max_norm=5.0, ema=A + 384, decay=0.9, warmup=1):
        return L.asr_adam_ema_step(p, g, m, v, lp, n, hyper, sumsq, max_norm, 0.9, 0.98, 1e-9, 1, ema, decay, warmup, none)

    def upd(p=A, ema=A + 64, n=8, decay=0.9, warmup=1, step=1.0):
        return L.asr_ema_update(p, ema, n, decay, warmup, step, none)

    for kw in (dict(p=none), dict(g=none), dict(m=none), dict(v=none), dict(hyper=none), dict(ema=none)):
        assert adam(**kw) == -1 and "asr_adam_ema_step: null pointer" in _lib.last_error(), kw
    assert adam(sumsq=none) == -1 and "clipping needs sumsq" in _lib.last_error()
    for kw in (dict(p=A + 4), dict(g=A + 8), dict(m=A + 12), dict(v=A + 20), dict(ema=A + 4), dict(ema=A + 8)):
        assert adam(**kw) == -1 and "16-byte aligned" in _lib.last_error(), kw
    for d in (0.0, 1.0, -0.5, 1.5, nan, inf, -inf):
        assert adam(decay=d) == -1 and "asr_adam_ema_step: decay" in _lib.last_error(), d
        assert upd(decay=d) == -1 and "asr_ema_update: decay" in _lib.last_error(), d
    for kw in (dict(p=none), dict(ema=none)):
        assert upd(**kw) == -1 and "asr_ema_update: null pointer" in _lib.last_error(), kw
    for kw in (dict(p=A + 4), dict(ema=A + 8)):
        assert upd(**kw) == -1 and "16-byte aligned" in _lib.last_error(), kw
    for s in (0.0, 0.5, -1.0, nan):
        assert upd(step=s) == -1 and "asr_ema_update: step" in _lib.last_error(), s


def test_kernels_wrappers_refuse_cpu_tensors():
    from asr_chinese_e2e_amd import kernels as K
    p, e = torch.zeros(8), torch.zeros(8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.ema_update(p, e, 0.9, 1)
    with pytest.raises(ValueError, match="float32"):
        K.ema_update(p.double(), e, 0.9, 1)
    h = torch.zeros(4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.adam_ema_step(p, p.clone(), p.clone(), p.clone(), None, h, None, 0.0, 0.9, 0.98, 1e-9, e, 0.9)
