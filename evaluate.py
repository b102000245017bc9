#!/usr/bin/env python3
"""evaluate.py - a test set in, its character error rate out: substitutions, deletions, insertions, sentence error rate, the oracle CER
of the n-best lists, the most frequent confusions and the worst tokens.

    python evaluate.py --model_name=TransformerOffical --ctc_weight=0.3 --ckpt=ckpt/exp/model.model --vocab_path=Predictor/vocab.t \
        --manifest=test.json --out=scores.jsonl

Model flags are train.py's (same parser and loading as transcribe.py).  Scoring flags:
  --ckpt, --vocab_path, --cmvn, --frontend, --resample, --batch_size     as transcribe.py's
  --manifest       one JSON object per line, {"wave": path, "tgt": transcript} - the collector format, which align.py also writes
  --search         transcribe (default: the search transcribe.py runs for the model's heads), ctc_prefix_beam or attention_beam
  --beam_size      the search's beam (5)
  --nbest          hypotheses kept per utterance (1); above 1 (ctc_prefix_beam, attention_beam) the summary gains the oracle CER: the
                   CER a perfect re-ranker of the lists would reach, and the histogram of the rank it would pick
  --consensus      1: the lists also go through consensus decoding (asr_chinese_e2e_amd/consensus.py) with the search's scores as the
                   posterior; the summary gains mbr_cer (the minimum-Bayes-risk entry), consensus_cer (the voted string) and mbr_rank_hist
  --posterior_scale   the scores are multiplied by it before the softmax that makes the weights (1.0)
  --rescore        a file tune.py wrote (or a JSON object {column: weight}): every n-best list is re-ranked by the weighted sum of its
                   columns before it is scored (asr_chinese_e2e_amd/rescore.py; ctc_prefix_beam or attention_beam).  If the weights name
                   the column "lm", --lm is the rescoring LM (an ARPA file, compiled with weight 1 and no insertion bonus, or an .npz
                   saved so) and is not forwarded to the search
  --joint, --blank_skip, --context, --context_score, --lm, --lm_weight, --lm_ins     forwarded to the search, as transcribe.py's
  --frame_topk     candidates per frame of ctc_prefix_beam (10)
  --out            a JSONL file: one line per utterance with its alignment spelled in tokens, then the summary
  --top            confusion pairs and tokens printed (10)
Prints the summary as one JSON line, then {"confusions": [...]} and {"worst_tokens": [...]}.  "cer" is token-level, (S + D + I) / the
reference tokens of the whole set; "cer_ref_convention" is the figure the training log prints (edit distance over the space-joined
strings, per utterance, averaged), for telling the two apart.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab, load_wav  # noqa: E402
from asr_chinese_e2e_amd.data_handler.loader import parser_norm  # noqa: E402
from asr_chinese_e2e_amd.data_handler import resample as resample_mod  # noqa: E402
from asr_chinese_e2e_amd.Utils import Pack  # noqa: E402
from train import TrainConfig, get_model_class, parse_flags  # noqa: E402
from transcribe import cmvn_path, load_model  # noqa: E402

CLI_KEYS = ("ckpt", "manifest", "search", "beam_size", "nbest", "joint", "blank_skip", "context", "context_score", "lm", "lm_weight", "lm_ins", "frame_topk",
            "out", "top", "cmvn", "frontend", "resample", "batch_size", "consensus", "posterior_scale", "rescore")
SEARCHES = ("transcribe", "ctc_prefix_beam", "attention_beam")


def read_manifest(path):
    """[(wave path, transcript)] of a collector file."""
    if not path or not os.path.isfile(str(path)):
        raise SystemExit(f"evaluate.py: give --manifest=<file of {{\"wave\", \"tgt\"}} lines> (got {path!r})")
    out = []
    with open(str(path), encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                rec = json.loads(line)
                out.append((str(rec["wave"]), str(rec["tgt"])))
            except (ValueError, KeyError, TypeError) as e:
                raise SystemExit(f"evaluate.py: {path} line {n}: not a {{\"wave\", \"tgt\"}} object ({e})") from e
    if not out:
        raise SystemExit(f"evaluate.py: {path} names no utterance")
    return out


def eval_options(cli):
    """The flags that can be judged before a model is loaded -> (search, nbest, beam, top); SystemExit for what is refused."""
    search = str(cli.get("search", "transcribe"))
    if search not in SEARCHES:
        raise SystemExit(f"evaluate.py: --search must be one of {', '.join(SEARCHES)} (got {search!r})")
    num = {}
    for flag, default in (("nbest", 1), ("beam_size", 5), ("top", 10), ("batch_size", 16), ("frame_topk", 10)):
        v = cli.get(flag, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < 1:
            raise SystemExit(f"evaluate.py: --{flag} must be a positive integer (got {v!r})")
        num[flag] = int(v)
    if num["nbest"] > 1 and search == "transcribe":
        raise SystemExit("evaluate.py: --nbest above 1 needs --search=ctc_prefix_beam or attention_beam (transcribe keeps the best hypothesis)")
    if num["nbest"] > num["beam_size"]:
        raise SystemExit(f"evaluate.py: --nbest={num['nbest']} above --beam_size={num['beam_size']}")
    num["consensus"] = int(bool(int(cli.get("consensus", 0) or 0)))
    if num["consensus"]:
        if search == "transcribe":
            raise SystemExit("evaluate.py: --consensus=1 needs --search=ctc_prefix_beam or attention_beam (it votes over an n-best list)")
        if num["nbest"] > 64:
            raise SystemExit(f"evaluate.py: --consensus=1 takes lists of at most 64 entries (--nbest={num['nbest']})")
    try:
        scale = float(cli.get("posterior_scale", 1.0))
    except (TypeError, ValueError):
        scale = float("nan")
    if not np.isfinite(scale) or scale <= 0.0:
        raise SystemExit(f"evaluate.py: --posterior_scale must be a finite number above 0 (got {cli.get('posterior_scale')!r})")
    num["posterior_scale"] = scale
    if cli.get("rescore") not in (None, "", False) and search == "transcribe":
        raise SystemExit("evaluate.py: --rescore needs --search=ctc_prefix_beam or attention_beam (it re-ranks an n-best list)")
    return search, num


def rescore_options(cli, vocab, V):
    """(weights, the rescoring LM or None) of --rescore; an --lm the weights use is taken out of cli, so the search does not get it."""
    if cli.get("rescore") in (None, "", False):
        return None, None
    from asr_chinese_e2e_amd.rescore import load_weights
    try:
        weights = load_weights(str(cli["rescore"]))
    except (OSError, ValueError) as e:
        raise SystemExit(f"evaluate.py: --rescore: {e}") from e
    lm = None
    if "lm" in weights:
        from asr_chinese_e2e_amd.lm import NgramLM
        path = cli.pop("lm", None)
        if path in (None, "", False):
            raise SystemExit("evaluate.py: the weights of --rescore name the column 'lm': give --lm=<ARPA file or .npz compiled with weight 1, ins 0>")
        try:
            lm = NgramLM.load(str(path), device="cuda") if str(path).endswith(".npz") else NgramLM.from_arpa(str(path), vocab, weight=1.0, ins=0.0, device="cuda")
            lm.check_vocab(V)
        except (OSError, ValueError) as e:
            raise SystemExit(f"evaluate.py: --lm: {e}") from e
    return weights, lm


def manifest_batches(entries, vocab, parser, bs, sample_rate, resample):
    """The packs model.evaluate takes, --batch_size utterances at a time: features from the front end, gold ids from the vocabulary."""
    for i in range(0, len(entries), bs):
        chunk = entries[i:i + bs]
        waves, rates = [], []
        for path, _ in chunk:
            pcm, sr = load_wav(path)
            if sr != sample_rate:
                if not resample:
                    raise SystemExit(f"evaluate.py: {path}: sample rate {sr}, the model expects {sample_rate}")
                try:
                    resample_mod.plan(sr)
                except ValueError as e:
                    raise SystemExit(f"evaluate.py: {path}: {e}") from e
            waves.append(pcm)
            rates.append(sr)
        S = max(1, max(len(w) for w in waves))
        wav = np.zeros((len(waves), S), dtype=np.float32)
        for b, w in enumerate(waves):
            wav[b, : len(w)] = w
        wav, wav_len = torch.from_numpy(wav), torch.tensor([len(w) for w in waves], dtype=torch.int32)
        if any(r != sample_rate for r in rates):
            wav, wav_len, _ = resample_mod.resample_batch(wav.cuda(), wav_len.tolist(), rates)
        feats, flen = parser.parse_batch(wav.cuda(), torch.as_tensor(wav_len, dtype=torch.int32).cuda())
        gold = [vocab.convert_str("".join(text.split()), use_bos=False, use_eos=False) for _, text in chunk]
        L = max(1, max(len(g) for g in gold))
        tgt = torch.zeros(len(gold), L, dtype=torch.int64)
        for b, g in enumerate(gold):
            tgt[b, : len(g)] = torch.tensor(g, dtype=torch.int64)
        yield Pack(wave=feats, wave_len=flen, tgt_for_input=tgt.cuda(), tgt_len=torch.tensor([len(g) for g in gold]).cuda(), key=[p for p, _ in chunk])


def search_options(cli, model, vocab, search):
    """The keywords the search takes beyond beam and nbest."""
    kw = {}
    runs_prefix_beam = search == "ctc_prefix_beam" or not model.use_decoder or str(cli.get("joint", "rescore")) == "ctc_rescore"
    if search != "ctc_prefix_beam" and cli.get("joint") not in (None, "", False):
        if str(cli["joint"]) not in ("rescore", "one_pass", "ctc_rescore"):
            raise SystemExit(f"evaluate.py: --joint must be rescore, one_pass or ctc_rescore (got {cli['joint']!r})")
        kw["joint"] = str(cli["joint"])
    if search == "ctc_prefix_beam":
        if not model.use_ctc:
            raise SystemExit("evaluate.py: --search=ctc_prefix_beam needs a model with the CTC head")
        kw["frame_topk"] = int(cli.get("frame_topk", 10))
    for flag in ("context", "lm", "blank_skip"):
        if cli.get(flag) not in (None, "", False) and not runs_prefix_beam:
            raise SystemExit(f"evaluate.py: --{flag} needs a search that runs the CTC prefix beam search: --search=ctc_prefix_beam, a CTC-only model or --joint=ctc_rescore")
    if cli.get("context") not in (None, "", False):
        from asr_chinese_e2e_amd.context import ContextGraph
        try:
            kw["context"] = ContextGraph.from_file(str(cli["context"]), vocab, score=float(cli.get("context_score", 3.0)), device="cuda")
        except (OSError, ValueError) as e:
            raise SystemExit(f"evaluate.py: --context: {e}") from e
    if cli.get("lm") not in (None, "", False):
        from asr_chinese_e2e_amd.lm import NgramLM
        if "context" in kw:
            raise SystemExit("evaluate.py: --lm and --context cannot be combined: the search runs one of the two")
        try:
            if str(cli["lm"]).endswith(".npz"):
                kw["lm"] = NgramLM.load(str(cli["lm"]), device="cuda")
            else:
                kw["lm"] = NgramLM.from_arpa(str(cli["lm"]), vocab, weight=float(cli.get("lm_weight", 0.3)), ins=float(cli.get("lm_ins", 0.0)), device="cuda")
            kw["lm"].check_vocab(model.V)
        except (OSError, ValueError) as e:
            raise SystemExit(f"evaluate.py: --lm: {e}") from e
    if cli.get("blank_skip") is not None and cli["blank_skip"] != "":
        from asr_chinese_e2e_amd.kernels import blank_skip_threshold
        try:
            if isinstance(cli["blank_skip"], bool):
                raise ValueError("a flag without a value")
            kw["blank_skip"] = float(cli["blank_skip"])
            blank_skip_threshold(kw["blank_skip"])
        except (TypeError, ValueError) as e:
            raise SystemExit(f"evaluate.py: --blank_skip must be a probability in (0, 1] (got {cli['blank_skip']!r})") from e
    return kw


def evaluate(**flags):
    cli = {k: flags.pop(k) for k in CLI_KEYS if k in flags}
    search, num = eval_options(cli)
    entries = read_manifest(cli.get("manifest"))
    config = TrainConfig()
    config.fn_build(flags)
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(flags)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py needs an MI355X: the searches and the scorer have no CPU fallback")
    vocab = Vocab.load(config.vocab_path)
    model = load_model(config, vocab, cli.get("ckpt"))
    parser = AudioParser(sample_rate=config.sample_rate, n_mels=config.n_mels, window_size=config.window_size,
                         lfr_m=config.lfr_m, lfr_n=config.lfr_n, frontend=str(cli.get("frontend", "reference")), **parser_norm(cmvn_path(cli)))
    weights, rescore_lm = rescore_options(cli, vocab, model.V)
    kw = search_options(cli, model, vocab, search)
    if weights is not None:
        kw.update(rescore=weights, rescore_lm=rescore_lm)
    batches = manifest_batches(entries, vocab, parser, num["batch_size"], config.sample_rate, bool(int(cli.get("resample", 0) or 0)))
    try:
        scorer = model.evaluate(batches, search=search, nbest=num["nbest"], beam_size=num["beam_size"], consensus=bool(num["consensus"]),
                                posterior_scale=num["posterior_scale"], **kw)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"evaluate.py: {e}") from e
    if cli.get("out") not in (None, "", False):
        scorer.write_jsonl(str(cli["out"]))
    print(json.dumps(scorer.summary(), ensure_ascii=False), flush=True)
    print(json.dumps({"confusions": scorer.confusions(num["top"])}, ensure_ascii=False), flush=True)
    print(json.dumps({"worst_tokens": scorer.per_token(num["top"])}, ensure_ascii=False), flush=True)


if __name__ == "__main__":
    evaluate(**parse_flags(sys.argv[1:]))
