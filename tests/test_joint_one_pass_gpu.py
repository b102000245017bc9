"""One-pass joint CTC / attention beam search on the device (asr_ctc_prefix_logprobs / asr_ctc_prefix_score / asr_ctc_prefix_gather /
asr_joint_beam_step, decode.one_pass_beam_search, model.beam_search(joint="one_pass"), transcribe) against the fp64 restatement of
tests/joint_ref.py, itself pinned by brute-force enumeration (tests/test_joint_prefix_cpu.py)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_model as R  # noqa: E402
from tests import joint_ref as J  # noqa: E402
from tests.helpers import ROOT  # noqa: E402
from tests.test_model_gpu import build, oracle_case, to_pack  # noqa: E402

DEV = "cuda"
SOS, EOS = 2, 3


def _close(a, b, tol=1e-4):
    if b == -math.inf or a == -math.inf:
        return a == b
    return abs(a - b) <= tol * max(1.0, abs(b))


# ---------------------------------------------------------------------------------------------------------- kernels
def _case(B, T, V, dtype, padded, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ld = V + 24 if padded else V
    buf = (torch.randn(B * T, ld, generator=g, device=DEV) * 2.0).to(dtype)
    logits = buf[:, :V].view(B, T, V)
    logp = J.log_softmax(logits.double().cpu().numpy())
    rng = np.random.default_rng(seed)
    in_len = [T] + [int(rng.integers(1, T + 1)) for _ in range(B - 1)]
    return logits, logp, in_len


def _candidates(rng, V, C, last):
    """C distinct ids: eos, blank and (where there is one) the hypothesis' last token among them, the rest random."""
    ids = [EOS, 0] + ([last] if last not in (None, EOS, 0) else [])
    rest = [c for c in rng.permutation(V).tolist() if c not in ids]
    return (ids + rest)[:C]


@pytest.mark.parametrize("dtype,padded,T,beam,C", [(torch.float32, False, 1, 1, 1), (torch.bfloat16, True, 37, 3, 5),
                                                   (torch.float32, True, 500, 8, 16), (torch.bfloat16, False, 2000, 4, 6)])
def test_prefix_score_kernel_matches_restatement(dtype, padded, T, beam, C):
    from asr_chinese_e2e_amd import kernels as K
    B, V = 2, 29
    lam = 0.4
    logits, logp, in_len = _case(B, T, V, dtype, padded, seed=T + beam)
    lpT = K.ctc_prefix_logprobs(logits)
    want_lp = np.transpose(logp, (0, 2, 1))
    assert np.abs(lpT.double().cpu().numpy() - want_lp).max() < 1e-4
    rng = np.random.default_rng(beam)
    Rn = B * beam
    in_len_d = torch.tensor(in_len, dtype=torch.int32, device=DEV)
    for step in (0, 1):
        # hypotheses: [sos] at step 0; otherwise random prefixes (repeated tokens included) of the utterance's lattice, some dead
        prefixes, alive = [], []
        for r in range(Rn):
            if step == 0:
                prefixes.append(())
                alive.append(r % beam == 0)
            else:
                n = int(rng.integers(1, 4))
                p = [int(x) for x in rng.integers(4, V, size=n)]
                if n > 1 and rng.random() < 0.5:
                    p[-1] = p[-2]
                prefixes.append(tuple(p))
                alive.append(r % 3 != 2)
        st_rb = torch.zeros(T, Rn, dtype=torch.float64)
        st_rt = torch.zeros(T, Rn, dtype=torch.float64)
        psi_g = torch.zeros(Rn, dtype=torch.float32)
        states = []
        for r, p in enumerate(prefixes):
            b = r // beam
            lp = logp[b, : in_len[b]]
            ps, (rn, rb) = J.prefix_state(lp, p)
            states.append((ps, (rn, rb)))
            alive[r] = alive[r] and ps > -math.inf                      # a live hypothesis of the search has psi > 0
            st_rb[: in_len[b], r] = torch.from_numpy(rb)
            st_rt[: in_len[b], r] = torch.from_numpy(np.logaddexp(rn, rb))
            psi_g[r] = ps
        last = [p[-1] if p else None for p in prefixes]
        ids = [_candidates(rng, V, C, last[r]) for r in range(Rn)]
        att = torch.from_numpy(-rng.exponential(2.0, size=(Rn, C))).float()
        last_tok = torch.tensor([l if l is not None else SOS for l in last], dtype=torch.int32, device=DEV)
        alive_d = torch.tensor(alive, dtype=torch.int32, device=DEV)
        att_ids = torch.tensor(ids, dtype=torch.int32, device=DEV)
        cand_rb = torch.full((T, Rn * C), float("nan"), dtype=torch.float64, device=DEV)
        cand_rt = torch.full_like(cand_rb, float("nan"))
        out = K.ctc_prefix_score(lpT, in_len_d, st_rb.to(DEV), st_rt.to(DEV), psi_g.to(DEV), last_tok, alive_d, att.to(DEV), att_ids,
                                 cand_rb, cand_rt, beam, step, lam, EOS)
        vals, oid, oatt, opsi, ofull = [t.cpu() for t in out]
        crb, crt = cand_rb.cpu().numpy(), cand_rt.cpu().numpy()
        for r in range(Rn):
            b = r // beam
            Tb = in_len[b]
            lp = logp[b, :Tb]
            ps_g, st_g = states[r]
            joint = []
            for j, c in enumerate(ids[r]):
                full, st = -math.inf, None
                if c == EOS:
                    psi = J.full_logprob(st_g, step == 0)
                else:
                    psi, st = J.extend(lp, st_g, last[r], c, step == 0)
                    full = J.full_logprob(st) if psi > -math.inf else -math.inf
                v = (1 - lam) * float(att[r, j]) + lam * (psi - float(psi_g[r])) if (alive[r] and psi > -math.inf) else -math.inf
                joint.append((v, j, c, psi, full))
                if alive[r] and c not in (EOS, 0):        # the candidate's state over the utterance's frames
                    rb, rt = st[1], np.logaddexp(st[0], st[1])
                    for got_s, want_s in ((crb[:Tb, r * C + j], rb), (crt[:Tb, r * C + j], rt)):
                        fin = np.isfinite(want_s)
                        assert np.array_equal(fin, np.isfinite(got_s)), (step, r, j)
                        assert np.all(np.abs(got_s[fin] - want_s[fin]) <= 1e-4 * np.maximum(1.0, np.abs(want_s[fin]))), (step, r, j)
            ranked = sorted(joint, key=lambda x: (-x[0], x[1]))[:beam]
            for k, (v, j, c, psi, full) in enumerate(ranked):
                assert int(oid[r, k]) == c, (step, r, k, ranked, oid[r])
                assert _close(float(vals[r, k]), v), (step, r, k, float(vals[r, k]), v)
                if alive[r]:
                    assert _close(float(opsi[r, k]), psi) and _close(float(ofull[r, k]), full), (step, r, k)
                    assert float(oatt[r, k]) == float(att[r, j])
        # gather: every live slot takes its parent's candidate state, found by token
        parent = torch.tensor([int(rng.integers(0, beam)) for _ in range(Rn)], dtype=torch.int32)
        pick = [int(rng.integers(0, C)) for _ in range(Rn)]
        new_tok = torch.tensor([ids[(r // beam) * beam + int(parent[r])][pick[r]] for r in range(Rn)], dtype=torch.int32)
        new_alive = torch.tensor([int(int(t) not in (EOS, 0) and alive[(r // beam) * beam + int(parent[r])]) for r, t in enumerate(new_tok)],
                                 dtype=torch.int32)
        dst_rb = torch.zeros(T, Rn, dtype=torch.float64, device=DEV)
        dst_rt = torch.zeros_like(dst_rb)
        K.ctc_prefix_gather(cand_rb, cand_rt, dst_rb, dst_rt, parent.to(DEV), new_tok.to(DEV), new_alive.to(DEV), att_ids, in_len_d, B, beam)
        drb, drt = dst_rb.cpu(), dst_rt.cpu()
        for r in range(Rn):
            if not new_alive[r]:
                assert float(drb[:, r].abs().max()) == 0.0
                continue
            col = ((r // beam) * beam + int(parent[r])) * C + pick[r]
            Tb = in_len[r // beam]
            assert np.array_equal(drb[:Tb, r].numpy(), crb[:Tb, col]) and np.array_equal(drt[:Tb, r].numpy(), crt[:Tb, col])


# ---------------------------------------------------------------------------------------------------------- whole search
def _oracle_model(dtype, lam):
    over = dict(d_model=64, hidden_size=64 if dtype == "bf16" else 16, num_head=2 if dtype == "bf16" else 4, ff_size=128, layer_num=2,
                ctc_weight=lam)
    cfg, sd, batch = oracle_case(3, 18, 16, 24, 5, over, seed=9)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 3.0      # peaked outputs: hypotheses end before maxlen
    if "decoder.tgt_word_prj.weight" in sd:                                             # tied: the state dict carries both names
        sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    sd["ctc_lo.weight"] = sd["ctc_lo.weight"] * 4.0
    model = build(cfg, 24, dtype=dtype).cuda()
    model.load_state_dict(sd)
    model.eval()
    return cfg, sd, batch, model


@pytest.mark.parametrize("dtype,beam,pre_beam,maxlen", [("fp32", 4, None, 10), ("fp32", 3, 8, 10), ("fp32", 4, None, 3), ("bf16", 3, None, 10)])
def test_one_pass_search_matches_restatement(dtype, beam, pre_beam, maxlen):
    """maxlen 10: hypotheses end by their own eos; maxlen 3: they reach the last step and get eos appended, with the CTC part
    replaced by the full-sequence probability (asr_joint_beam_step's rec_end 2 path)."""
    lam, nbest = 0.5, 3
    cfg, sd, batch, model = _oracle_model(dtype, lam)
    pack = to_pack(batch)
    got = model.beam_search(pack, beam, nbest, maxlen, ctc_weight=lam, joint="one_pass", ctc_pre_beam=pre_beam)
    C = pre_beam or min(16, int(1.5 * beam))
    enc = R.encoder_forward(sd, cfg, batch["wave"], batch["wave_len"])
    nonempty = forced = 0
    for b in range(3):
        Tb = int(batch["wave_len"][b])
        e = enc[b: b + 1, :Tb]
        logp = J.log_softmax(R.ctc_logits(sd, e[0]).double().numpy())

        def att_of(seq, e=e):
            return R.decoder_step_logits(sd, cfg, torch.tensor([seq]), e).double().numpy()

        want = J.one_pass_search(att_of, logp, beam, C, maxlen, lam, SOS, EOS, nbest=nbest)
        assert len(got[b]) == len(want)            # both empty when the attention candidates never include a spellable end
        nonempty += len(want) > 0
        forced += sum(len(w["yseq"]) == maxlen + 2 for w in want)       # sos, maxlen tokens, appended eos
        if not want:
            continue
        if dtype == "fp32":
            for h, w in zip(got[b], want):
                assert h["yseq"] == w["yseq"], (b, got[b], want)
                for k in ("score", "att_score", "ctc_score"):
                    assert _close(h[k], w[k]), (b, k, h, w)
        else:
            err = abs(got[b][0]["score"] - want[0]["score"]) / max(1.0, abs(want[0]["score"]))
            assert err < 0.2, (got[b][0], want[0])      # the gate of test_beam_search_matches_oracle's bf16 case
    assert nonempty > 0 or dtype == "bf16"
    assert forced > 0 or maxlen > 3


@pytest.mark.parametrize("maxlen", [10, 3])
def test_one_pass_scores_are_consistent(maxlen):
    """ctc_score = -nll of the training CTC kernel, att_score = plain beam search's score of the same yseq, score = their mix.
    maxlen 3 reaches the forced end: eos appended at the last step, ctc_score the full-sequence probability."""
    from asr_chinese_e2e_amd import kernels as K
    lam, beam = 0.3, 5
    cfg, sd, batch, model = _oracle_model("fp32", lam)
    pack = to_pack(batch)
    got = model.beam_search(pack, beam, beam, maxlen, ctc_weight=lam, joint="one_pass")
    plain = model.beam_search(pack, beam, beam, maxlen)
    with torch.no_grad():
        logits = model.forward(pack).ctc_logits.contiguous()
    seen = forced = 0
    for b in range(3):
        att_of = {tuple(h["yseq"]): h["score"] for h in plain[b]}
        forced += sum(len(h["yseq"]) == maxlen + 2 for h in got[b])
        for h in got[b]:
            toks = h["yseq"][1:-1]
            assert h["yseq"][0] == SOS and h["yseq"][-1] == EOS and 0 not in toks
            lab = torch.tensor([toks or [0]], dtype=torch.int32, device=DEV)
            nll, _ = K.ctc_fwd_bwd(logits[b:b + 1], batch["wave_len"][b:b + 1].to(torch.int32).to(DEV), lab,
                                   torch.tensor([len(toks)], dtype=torch.int32, device=DEV), model._engine.ws, want_grad=False)
            assert _close(h["ctc_score"], -float(nll[0])), (b, h, -float(nll[0]))
            assert abs(h["score"] - (lam * h["ctc_score"] + (1 - lam) * h["att_score"])) <= 1e-4 * max(1.0, abs(h["score"]))
            if tuple(h["yseq"]) in att_of:
                seen += 1
                assert _close(h["att_score"], att_of[tuple(h["yseq"])]), (b, h)
        assert all(got[b][i]["score"] >= got[b][i + 1]["score"] for i in range(len(got[b]) - 1))
    assert seen > 0
    assert forced > 0 or maxlen > 3


# ---------------------------------------------------------------------------------------------------------- what rescoring cannot do
def _cer(hyps, labels):
    err = sum(R.edit_distance(h, l) for h, l in zip(hyps, labels))
    return 100.0 * err / sum(len(l) for l in labels)


def test_one_pass_recovers_transcripts_of_an_audio_blind_decoder(deterministic_mode):
    """A joint model memorises four utterances (as test_train_loop_gpu's overfit test); zeroing the decoder's cross-attention output
    projection then makes the attention head an audio-blind language model while the CTC head stays intact.  Two-pass rescoring can
    only choose among audio-independent hypotheses; one-pass search (ctc_weight 0.5, beam 8, pre_beam 16) must do strictly better
    and return the transcripts - and on the intact model it must return them too."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    torch.manual_seed(0)
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0, ctc_weight=0.3,
                      dtype="fp32", cross_mask="wave_len", cer_in_iterate=False))
    model = M(cfg, Vocab.synthetic(20)).cuda()
    opt = NoamOpt(64, 1, 60, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    pack = synthetic_pack(4, 40, 16, 20, seed=3, ragged=True, Lmin=3, Lmax=6, device="cuda")
    labels = [[int(t) for t in row if int(t) != 0] for row in pack.tgt_for_input.cpu()]

    def one_pass(m):
        return [h[0]["yseq"][1:-1] if h else [] for h in m.beam_search(pack, 8, 1, 10, ctc_weight=0.5, joint="one_pass", ctc_pre_beam=16)]

    model.train()
    steps, ok = 0, False
    while steps < 3000 and not ok:
        for _ in range(200):
            model.iterate(pack, optimizer=opt)
        steps += 200
        model.eval()
        ok = (model.ctc_greedy_search(pack) == labels and
              [h[0]["yseq"][1:-1] for h in model.beam_search(pack, beam_size=3, nbest=1, decode_max_len=10)] == labels)
        model.train()
    assert ok, steps
    for _ in range(800):                            # beyond the first exact decode: a confident CTC head
        model.iterate(pack, optimizer=opt)
    model.eval()
    assert one_pass(model) == labels
    sd = {k: (torch.zeros_like(v) if ".enc_attn.fc." in k else v) for k, v in model.state_dict().items()}
    assert sum(".enc_attn.fc." in k for k in sd) == 4           # weight and bias of both layers
    model.load_state_dict(sd)                                     # refreshes the engine's low-precision / transposed copies
    rescored = [h[0]["yseq"][1:-1] if h else [] for h in model.beam_search(pack, 8, 1, 10, ctc_weight=0.5)]
    blind = one_pass(model)
    assert _cer(blind, labels) < _cer(rescored, labels), (blind, rescored, labels)
    assert blind == labels, (blind, labels)


# ---------------------------------------------------------------------------------------------------------- public surface
def test_one_pass_surface_checks():
    cfg, sd, batch, model = _oracle_model("fp32", 0.3)
    pack = to_pack(batch)
    with pytest.raises(ValueError):
        model.beam_search(pack, 3, 1, 6, ctc_weight=0.0, joint="one_pass")
    with pytest.raises(ValueError):
        model.beam_search(pack, 4, 1, 6, ctc_weight=0.3, joint="one_pass", ctc_pre_beam=3)
    with pytest.raises(ValueError):
        model.beam_search(pack, 4, 1, 6, ctc_weight=0.3, joint="two_pass")
    att_only = build(R.default_cfg(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1), 24,
                     "TransformerOffical", dtype="fp32").cuda()
    with pytest.raises(RuntimeError):
        att_only.beam_search(pack, 2, 1, 4, ctc_weight=0.3, joint="one_pass")
    ctc_only = build(R.default_cfg(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, ctc_weight=1.0), 24,
                     "TransformerCTC", dtype="fp32").cuda()
    with pytest.raises(RuntimeError):
        ctc_only.beam_search(pack, 2, 1, 4, ctc_weight=0.3, joint="one_pass")
    with pytest.raises(RuntimeError):
        ctc_only.transcribe(pack, joint="one_pass")


def test_transcribe_one_pass_and_defaults():
    from asr_chinese_e2e_amd.Utils import Pack
    cfg, sd, batch, model = _oracle_model("fp32", 0.3)
    full = to_pack(batch)
    audio = Pack(wave=full.wave, wave_len=full.wave_len)
    got = model.transcribe(audio, beam_size=4, joint="one_pass")
    want = model.beam_search(full, 4, 1, ctc_weight=0.3, joint="one_pass")
    assert [r["ids"] for r in got] == [h[0]["yseq"][1:-1] if h else [] for h in want]
    for r in got:
        assert isinstance(r["text"], str) and [t["id"] for t in r["tokens"]] == r["ids"]
    # the default call is the two-pass search, unchanged
    assert [r["ids"] for r in model.transcribe(audio, beam_size=4)] == \
        [h[0]["yseq"][1:-1] for h in model.beam_search(full, 4, 1, ctc_weight=0.3)]
    assert model.beam_search(full, 4, 2, 8, ctc_weight=0.3) == model.beam_search(full, 4, 2, 8, ctc_weight=0.3, joint="rescore")


def test_transcribe_cli_one_pass(tmp_path):
    from asr_chinese_e2e_amd.data_handler import Vocab
    from tests.test_ctc_align_gpu import _write_wav
    sys.path.insert(0, ROOT)
    from train import TrainConfig, get_model_class
    flags = dict(model_name="TransformerOffical", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32",
                 ctc_weight=0.3)
    config = TrainConfig()
    config.fn_build(flags)
    Model, MC = get_model_class(config.model_name)
    config.fn_combine(MC())
    config.fn_build(flags)
    vocab = Vocab.synthetic(40)
    vocab.save(str(tmp_path / "vocab.t"))
    torch.manual_seed(0)
    Model(config, vocab).save(str(tmp_path / "m.model"))
    wavs = [tmp_path / "a.wav", tmp_path / "b.wav"]
    for i, (p, s) in enumerate(zip(wavs, [1.1, 0.6])):
        _write_wav(p, s, i)
    cmd = [sys.executable, os.path.join(ROOT, "transcribe.py")] + [f"--{k}={v}" for k, v in flags.items()] + \
        [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}", "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3",
         "--joint=one_pass"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [l["file"] for l in lines] == [str(p) for p in wavs]
    for line in lines:
        assert isinstance(line["text"], str) and isinstance(line["ids"], list)
