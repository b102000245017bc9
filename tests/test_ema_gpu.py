"""The exponential moving average of the parameters on the GPU, bit for bit against tests/ema_ref.py (no tolerance anywhere): the fused
Adam + EMA kernel and the stand-alone pass at the sizes of test_rowwise_states_gpu's Adam tests, the model's average over real training
steps (fused optimizer, stock optimizers, captured graph, two ranks), ema_weights(), the trainer's checkpoints, and averaging on load.
Needs a real MI355X: run with `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ema_ref as E  # noqa: E402
from tests.helpers import ROOT, free_port  # noqa: E402

DEV = "cuda"
SENT = 64
BF16 = torch.bfloat16
SIZES = [1, 2, 3, 100003, 2097152 + 4 * 77 + 3]      # the tail alone (x3); one trip + a tail of 3; a second grid-stride trip of 77 vectors + the tail


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({torch.float32: torch.int32, BF16: torch.int16}.get(t.dtype, t.dtype))


def same_bits(a, b):
    if isinstance(b, np.ndarray):
        b = torch.from_numpy(np.ascontiguousarray(b))
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(data, sentinel):
    """data (flat, CPU) at the front of a device allocation with SENT sentinel elements behind it: (view, whole buffer)."""
    buf = torch.full((data.numel() + SENT,), sentinel, dtype=data.dtype)
    buf[:data.numel()] = data
    buf = buf.to(DEV)
    return buf[:data.numel()], buf


def untouched(buf, n, sentinel):
    tail = buf[n:].cpu()
    return tail.numel() == SENT and same_bits(tail, torch.full((SENT,), sentinel, dtype=buf.dtype))


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    return (p, torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.1,
            p + torch.randn(n, generator=g) * 0.05)      # p, g, m, v, ema (an average some way from p)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", SIZES)
def test_adam_ema_step_bits(K, n):
    """Every case: p, g, m, v, lp have the bits of K.adam_step on clones of the same inputs; ema has the bits of ema_ref applied to the
    kernel's own p; the sentinels behind all six buffers are untouched."""
    b1, b2, lr = 0.9, 0.98, 1e-2
    p0, g0, m0, v0, e0 = _state(n, n % 1000 + 7)
    norm = float(torch.sqrt((g0.double() ** 2).sum()))
    ws = K.Workspace(DEV)
    sumsq = torch.zeros(1, device=DEV)
    ncase = 0
    for warmup, s in ((True, 1), (True, 50), (False, 50)):
        for max_norm in (0.25 * norm, 4.0 * norm):                       # clipping active / inactive
            for write_clipped in (True, False):
                for with_lp in (True, False):
                    hyper = torch.tensor([lr, 1 - b1 ** s, (1 - b2 ** s) ** 0.5, s], dtype=torch.float32, device=DEV)
                    ref = [guarded(x, 1.0 + i)[0] for i, x in enumerate((p0, g0, m0, v0))]
                    ref_lp = guarded(torch.zeros(n, dtype=BF16), 5.0)[0]
                    K.grad_sumsq(ref[1], sumsq, ws)
                    K.adam_step(*ref, ref_lp if with_lp else None, hyper, sumsq, max_norm, b1, b2, 1e-9, write_clipped=write_clipped)
                    (P, Pb), (G, Gb), (M_, Mb), (V_, Vb), (Em, Eb) = (guarded(x, 11.0 + i) for i, x in enumerate((p0, g0, m0, v0, e0)))
                    lp, lpb = guarded(torch.zeros(n, dtype=BF16), 16.0)
                    K.adam_ema_step(P, G, M_, V_, lp if with_lp else None, hyper, sumsq, max_norm, b1, b2, 1e-9, Em, 0.999, warmup,
                                    write_clipped=write_clipped)
                    tag = (n, warmup, s, max_norm > norm, write_clipped, with_lp)
                    for got, want, name in zip((P, G, M_, V_, lp), (*ref, ref_lp), "pgmvl"):
                        assert same_bits(got, want), (name, tag)
                    assert not same_bits(P, p0) and same_bits(G, g0) == (not (write_clipped and max_norm < norm)), tag
                    want = E.ema_update(e0.numpy(), P.cpu().numpy(), 0.999, s, warmup)
                    assert same_bits(Em, want), ("ema", tag)
                    assert not same_bits(Em, e0), tag
                    for i, buf in enumerate((Pb, Gb, Mb, Vb, Eb)):
                        assert untouched(buf, n, 11.0 + i), (i, tag)
                    assert untouched(lpb, n, 16.0), tag
                    ncase += 1
    assert ncase == 24


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_bits(K, n):
    p0, _, _, _, e0 = _state(n, n % 1000 + 3)
    for decay, warmup, s in ((0.999, True, 1), (0.999, True, 50), (0.999, False, 50), (0.9, True, 8991), (0.5, False, 1)):
        (P, Pb), (Em, Eb) = guarded(p0, 21.0), guarded(e0, 22.0)
        out = K.ema_update(P, Em, decay, s, warmup)
        assert out is Em
        assert same_bits(P, p0), "p is only read"
        assert same_bits(Em, E.ema_update(e0.numpy(), p0.numpy(), decay, s, warmup)), (n, decay, warmup, s)
        assert untouched(Pb, n, 21.0) and untouched(Eb, n, 22.0)
    # the fixed point: an average equal to p stays equal to p
    (P, _), (Em, _) = guarded(p0, 21.0), guarded(p0, 22.0)
    K.ema_update(P, Em, 0.999, 7, True)
    assert same_bits(Em, p0)


def test_launchers_refuse_before_launching(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    n = 64
    p, g, m, v, e = (x.to(DEV) for x in _state(n, 1))
    hyper = torch.tensor([1e-2, 0.1, 0.1, 1.0], device=DEV)
    before = [x.clone() for x in (p, g, m, v, e)]
    for decay in (0.0, 1.0, float("nan")):
        with pytest.raises(AsrHipError, match="decay"):
            K.adam_ema_step(p, g, m, v, None, hyper, None, 0.0, 0.9, 0.98, 1e-9, e, decay)
        with pytest.raises(AsrHipError, match="decay"):
            K.ema_update(p, e, decay, 1)
    with pytest.raises(AsrHipError, match="step"):
        K.ema_update(p, e, 0.9, 0)
    with pytest.raises(AsrHipError, match="16-byte aligned"):
        K.ema_update(p[1:33], e[:32], 0.9, 1)
    with pytest.raises(AsrHipError, match="16-byte aligned"):
        K.adam_ema_step(p[:32], g[:32], m[:32], v[:32], None, hyper, None, 0.0, 0.9, 0.98, 1e-9, e[1:33], 0.9)
    assert all(same_bits(a, b) for a, b in zip((p, g, m, v, e), before))


# ------------------------------------------------------------------------------------------------ model
def small_model(dtype="fp32", seed=0, cls="TransformerOffical", **extra):
    """tests/test_train_loop_gpu.small_model's shape (d_model 64, 2 layers), with the keys of this feature."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    torch.manual_seed(seed)
    M = getattr(Models, cls)
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0,
                      ctc_weight=0.3, dtype=dtype, num_epoch=2, warm_up=10, **extra))
    return M(cfg, Vocab.synthetic(40)), cfg


def batches(n, seed=0, dtype=torch.float32):
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    return [synthetic_pack(4, 24, 16, 40, seed=seed + i, ragged=True, Lmin=2, Lmax=6, device="cuda", dtype=dtype) for i in range(n)]


def fused_opt(model, cfg):
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    return NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))


def gaps_zero(flat, buf):
    keep = torch.ones(flat.numel, dtype=torch.bool)
    for s, e in flat.block_range:
        keep[s:e] = False
    return int(keep.sum()) > 0 and float(buf.cpu()[keep].abs().max()) == 0.0


def _follow(model, step_fn, steps, decay, warmup=True, first_step=1):
    """Run `steps` steps; after each, flat.ema must equal ema_ref folded over the run's OWN snapshots of flat.p (no determinism needed)."""
    flat = model._flat
    e = flat.ema.cpu().numpy().copy()
    for k in range(steps):
        before = flat.p.clone()
        step_fn(k)
        p = flat.p.cpu().numpy()
        assert not same_bits(flat.p, before), "the step moved the parameters"
        e = E.ema_update(e, p, decay, first_step + k, warmup)
        assert same_bits(flat.ema, e), f"step {first_step + k}"
        assert not same_bits(flat.ema, flat.p)
    assert gaps_zero(flat, flat.ema) and gaps_zero(flat, flat.p)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("warmup", [True, False])
def test_model_average_follows_the_fused_step(dtype, warmup):
    model, cfg = small_model(dtype, ema_decay=0.9, ema_warmup=warmup)
    model = model.cuda()
    opt = fused_opt(model, cfg)
    data = batches(5, dtype=torch.float32 if dtype == "fp32" else BF16)
    model._ensure_engine("cuda")
    flat = model._flat
    assert flat.ema is not None and flat.ema.dtype == torch.float32 and flat.ema.numel() == flat.numel
    assert same_bits(flat.ema, flat.p), "the average starts as a copy of p"
    _follow(model, lambda k: model.iterate(data[k], optimizer=opt), 5, 0.9, warmup)
    assert opt._step == 5


def test_model_without_average_allocates_nothing():
    model, cfg = small_model("fp32")
    model = model.cuda()
    opt = fused_opt(model, cfg)
    model.iterate(batches(1)[0], optimizer=opt)
    assert model._flat.ema is None and model.ema_decay == 0.0


@pytest.mark.parametrize("kind", ["sgd", "noam_over_adam"])
def test_model_average_with_stock_optimizers(kind):
    """Optimizers that do not run the fused Adam pass: the stand-alone kernel, with the model's own step count (SGD keeps none) or
    NoamOpt's."""
    from asr_chinese_e2e_amd.Trainer import NoamOpt
    model, cfg = small_model("fp32", ema_decay=0.9)
    model = model.cuda()
    if kind == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
    else:
        opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, torch.optim.Adam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    data = batches(5)
    model._ensure_engine("cuda")
    _follow(model, lambda k: model.iterate(data[k], optimizer=opt), 5, 0.9)


def test_average_leaves_the_trajectory_alone(deterministic_mode):
    def run(**extra):
        model, cfg = small_model("fp32", **extra)
        model = model.cuda()
        opt = fused_opt(model, cfg)
        for b in batches(3):
            model.iterate(b, optimizer=opt)
        return model._flat.p.clone(), model._flat.m.clone(), model._flat.v.clone()
    a, b = run(), run()
    assert all(same_bits(x, y) for x, y in zip(a, b)), "precondition: two runs without an average from one seed have equal bits"
    c = run(ema_decay=0.999)
    assert all(same_bits(x, y) for x, y in zip(a, c)), "the average changed the parameters or Adam's moments"


def test_graphed_step_average():
    from asr_chinese_e2e_amd.graph import GraphedStep
    model, cfg = small_model("fp32", ema_decay=0.9)
    model = model.cuda()
    opt = fused_opt(model, cfg)
    data = batches(1)[0]
    model.iterate(data, optimizer=opt)               # one eager step: the average now differs from p
    flat = model._flat
    assert not same_bits(flat.ema, flat.p)
    before = (flat.ema.clone(), flat.p.clone())
    g = GraphedStep(model, opt, data)                # two warm-up steps and the capture, on a snapshot
    torch.cuda.synchronize()
    assert same_bits(flat.ema, before[0]) and same_bits(flat.p, before[1]), "warm-up and capture left a trace"
    _follow(model, lambda k: g(data), 3, 0.9, first_step=2)      # three replays: the step is read from the device
    assert opt._step == 4


def _logits(model, pack):
    with torch.no_grad():
        return model.forward(pack).ctc_logits.clone()


def test_ema_weights_round_trip(tmp_path, deterministic_mode):
    model, cfg = small_model("bf16", ema_decay=0.9)
    model = model.cuda().eval()
    opt = fused_opt(model, cfg)
    data = batches(4, dtype=BF16)
    model.train()
    for b in data[:3]:
        model.iterate(b, optimizer=opt)
    model.eval()
    flat = model._flat
    path = str(tmp_path / "avg.ema.model")
    model.save_ema(path)
    sd = torch.load(path, weights_only=True)
    assert list(sd.keys()) == list(model.state_dict().keys())
    assert same_bits(sd["decoder.tgt_word_prj.weight"], sd["decoder.tgt_word_emb.weight"])
    for name, (off, shape) in flat.index.items():
        assert same_bits(sd[name], flat.view(flat.ema, name)), name
    fresh, _ = small_model("bf16", seed=5)           # no average of its own: the file is a plain state dict
    fresh.load(path)
    fresh = fresh.cuda().eval()
    want_avg = _logits(fresh, data[3])
    state = [t.clone() for t in (flat.p, flat.ema, flat.m, flat.v, flat.lp)]
    raw = _logits(model, data[3])
    version = flat.version
    with model.ema_weights() as m_:
        assert m_ is model and flat.version > version
        inside = _logits(model, data[3])
        assert same_bits(flat.p, state[1]) and same_bits(flat.ema, state[0])
        assert same_bits(flat.lp, state[1].bfloat16())
        with pytest.raises(RuntimeError, match="ema_weights"):
            model.iterate(data[0], optimizer=opt, is_train=True)
        from asr_chinese_e2e_amd.graph import GraphedModel
        with pytest.raises(RuntimeError, match="ema_weights"):
            GraphedModel(model).iterate(data[0], optimizer=opt)
        with pytest.raises(RuntimeError, match="ema_weights"):
            model.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="ema_weights"):
            model.load_ema(path)
        with pytest.raises(RuntimeError, match="already active"):
            with model.ema_weights():
                pass
        ev, _ = model.iterate(data[3], is_train=False)          # evaluation runs on the average
        assert np.isfinite(float(ev.loss))
        inside_sd = model.ema_state_dict()
    assert same_bits(inside, want_avg) and not same_bits(inside, raw)
    assert all(same_bits(inside_sd[k], sd[k]) for k in sd)
    assert same_bits(_logits(model, data[3]), raw)
    for t, s in zip((flat.p, flat.ema, flat.m, flat.v, flat.lp), state):
        assert same_bits(t, s)
    # a step taken after a round trip equals a step taken without one
    twin, tcfg = small_model("bf16", ema_decay=0.9)
    twin = twin.cuda()
    topt = fused_opt(twin, tcfg)
    for b in data[:3]:
        twin.iterate(b, optimizer=topt)
    assert same_bits(twin._flat.p, flat.p), "precondition: deterministic mode reproduces the three steps"
    model.train()
    model.iterate(data[3], optimizer=opt)
    twin.iterate(data[3], optimizer=topt)
    assert same_bits(model._flat.p, twin._flat.p) and same_bits(model._flat.ema, twin._flat.ema)
    # load / load_ema
    model.load_state_dict(sd)
    assert same_bits(flat.ema, flat.p), "load_state_dict resets the average to the loaded weights"
    model.save(str(tmp_path / "w.model"))
    twin.save_ema(str(tmp_path / "t.ema.model"))
    model.load(str(tmp_path / "w.model"))
    model.load_ema(str(tmp_path / "t.ema.model"))
    assert same_bits(flat.ema, twin._flat.ema) and not same_bits(flat.ema, flat.p)
    short = {k: v for k, v in sd.items() if k != "ctc_lo.bias"}
    torch.save(short, str(tmp_path / "short.model"))
    with pytest.raises(KeyError, match="ctc_lo.bias"):
        model.load_ema(str(tmp_path / "short.model"))
    # a model without an average refuses
    plain, _ = small_model("bf16")
    plain = plain.cuda()
    with pytest.raises(RuntimeError, match="ema_decay is 0"):
        with plain.ema_weights():
            pass


def test_average_survives_a_device_move():
    model, cfg = small_model("fp32", ema_decay=0.9)
    model = model.cuda()
    opt = fused_opt(model, cfg)
    for b in batches(2):
        model.iterate(b, optimizer=opt)
    ema = model._flat.ema.clone()
    model = model.cuda()                  # _apply: the views are re-validated; a rebuilt buffer must carry the average
    model._views_checked = False
    for _, p in model.named_parameters():
        p.data = p.data.clone()           # the parameters leave the flat buffer: _ensure_engine rebuilds it
    model._ensure_engine("cuda")
    assert same_bits(model._flat.ema, ema) and not same_bits(model._flat.ema, model._flat.p)


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_writes_evaluates_and_resumes_the_average(tmp_path):
    from asr_chinese_e2e_amd.Trainer import Trainer11
    model, cfg = small_model("fp32", ema_decay=0.9)
    model = model.cuda()
    opt = fused_opt(model, cfg)
    data = batches(3)
    tr = Trainer11(opt, model, data, dev_iter=data[:1], test_iter=data[:1], ckpt_root=str(tmp_path), exp_name="exp", log_every_iter=1,
                   eval_every_iter=2, save_every_iter=3)
    tr.train()                                   # 2 epochs x 3 steps, as test_trainer_checkpoint_and_eval
    assert tr.global_step == 6
    tags = {h["tag"] for h in tr.history}
    assert {"dev/loss", "dev/ema/loss", "dev/ema/cer", "test/ema/loss", "test/loss"} <= tags
    raw = [h["value"] for h in tr.history if h["tag"] == "dev/loss"]
    avg = [h["value"] for h in tr.history if h["tag"] == "dev/ema/loss"]
    assert len(raw) == len(avg) and all(np.isfinite(avg)) and raw != avg
    keys = list(model.state_dict().keys())
    for prefix in ("e0_s3", "e1_s6"):
        f = tmp_path / "exp" / (prefix + ".ema.model")
        assert os.path.isfile(f) and os.path.isfile(tmp_path / "exp" / (prefix + ".model"))
        assert list(torch.load(str(f), weights_only=True).keys()) == keys
    assert model.training
    # resume into a fresh model that has no flat buffers yet
    m2, cfg2 = small_model("fp32", seed=1, ema_decay=0.9)
    m2 = m2.cuda()
    t2 = Trainer11(fused_opt(m2, cfg2), m2, data, ckpt_root=str(tmp_path), exp_name="exp2")
    t2.load_from_ckpt("exp", 1, 6)
    assert same_bits(m2._flat.ema, model._flat.ema) and same_bits(m2._flat.p, model._flat.p)
    assert not same_bits(m2._flat.ema, m2._flat.p)
    # without the file the average restarts from the loaded weights
    os.remove(tmp_path / "exp" / "e1_s6.ema.model")
    m3, cfg3 = small_model("fp32", seed=2, ema_decay=0.9)
    m3 = m3.cuda()
    t3 = Trainer11(fused_opt(m3, cfg3), m3, data, ckpt_root=str(tmp_path), exp_name="exp3")
    t3.load_from_ckpt("exp", 1, 6)
    assert same_bits(m3._flat.ema, m3._flat.p) and same_bits(m3._flat.p, model._flat.p)
    # eval_ema=False: no second pass
    t4 = Trainer11(opt, model, data[:1], dev_iter=data[:1], ckpt_root=str(tmp_path), exp_name="exp4", eval_ema=False)
    t4.evaluate(data[:1], "dev/")
    assert any(h["tag"] == "dev/loss" for h in t4.history) and not any("ema/" in h["tag"] for h in t4.history)


# ------------------------------------------------------------------------------------------------ two ranks
DP2_EMA_WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
from asr_chinese_e2e_amd import Models, dist as D
from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
from asr_chinese_e2e_amd.Utils import Pack
rank, world = D.init("gloo")          # two ranks share the one GPU of the test box: gloo moves the CUDA buckets
torch.cuda.set_device(0)
torch.manual_seed(10 + rank)          # the ranks start from DIFFERENT weights: the broadcast makes them replicas
M = Models.TransformerOffical
cfg = M.get_default_config()()
cfg.fn_build(dict(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0, ctc_weight=0.3, dtype="fp32",
                  ema_decay=0.9))
m = M(cfg, Vocab.synthetic(40)).cuda()
opt = NoamOpt(64, 1, 10, FusedAdam(m.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
dp = D.DataParallel(m, "cuda", bucket_bytes=64 << 10)
assert torch.equal(m._flat.ema.view(torch.int32), m._flat.p.view(torch.int32))
full = synthetic_pack(6, 24, 16, 40, seed=5, ragged=True, Lmin=2, Lmax=6, device="cuda")
lo, hi = (0, 3) if rank == 0 else (3, 6)
mine = Pack()
mine.add(**{k: full[k][lo:hi].contiguous() for k in ("wave", "wave_len", "tgt_for_input", "tgt_for_metric", "tgt_len")})
for _ in range(3):
    dp.iterate(mine, optimizer=opt)
torch.cuda.synchronize()
assert not torch.equal(m._flat.ema, m._flat.p)
def gathered(t):                      # on the CPU: gloo gathers no CUDA tensors
    t = t.cpu()
    out = [torch.empty_like(t) for _ in range(world)]
    torch.distributed.all_gather(out, t)
    return [o.view(torch.int32) for o in out]
both = gathered(m._flat.ema)
assert torch.equal(both[0], both[1]), "the ranks' averages differ"
ps = gathered(m._flat.p)
assert torch.equal(ps[0], ps[1]), "the ranks' parameters differ"
torch.distributed.barrier(); torch.distributed.destroy_process_group()
print("rank", rank, "dp2 ema ok")
"""


def test_two_ranks_keep_one_average(tmp_path):
    script = tmp_path / "dp2_ema_worker.py"
    script.write_text(DP2_EMA_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=free_port(), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} dp2 ema ok" in o


# ------------------------------------------------------------------------------------------------ averaging on load
def test_load_model_averages_a_list_of_checkpoints(tmp_path):
    import transcribe as T_
    from asr_chinese_e2e_amd.averaging import average_state_dicts
    from asr_chinese_e2e_amd.data_handler import Vocab
    paths = []
    for i in range(3):
        m, cfg = small_model("bf16", seed=20 + i)
        paths.append(str(tmp_path / f"e0_s{i}.model"))
        m.save(paths[-1])
    cfg.fn_build(dict(model_name="TransformerOffical"))
    want = average_state_dicts(paths)
    model = T_.load_model(cfg, Vocab.synthetic(40), ",".join(paths))
    assert not model.training and next(model.parameters()).is_cuda
    got = model.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert not same_bits(got["encoder.linear_in.weight"], torch.load(paths[0], weights_only=True)["encoder.linear_in.weight"])
    one = T_.load_model(cfg, Vocab.synthetic(40), paths[1])
    assert same_bits(one.state_dict()["encoder.linear_in.weight"], torch.load(paths[1], weights_only=True)["encoder.linear_in.weight"])
    with pytest.raises(SystemExit, match="checkpoint not found"):
        T_.load_model(cfg, Vocab.synthetic(40), paths[0] + "," + str(tmp_path / "missing.model"))
