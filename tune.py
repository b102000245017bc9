#!/usr/bin/env python3
"""tune.py - a dev set in, the rescoring weights of its n-best lists out: every utterance goes through the search once, and a grid of
weight vectors is swept over the lists on the GPU (asr_chinese_e2e_amd/rescore.py).

    python tune.py --model_name=TransformerOffical --ctc_weight=0.3 --ckpt=ckpt/exp/model.model --vocab_path=Predictor/vocab.t \
        --manifest=dev.json --search=attention_beam --beam_size=10 --nbest=10 --lm=lm.arpa \
        --grid="att_score=1;ctc_score=0:1:0.25;lm=0:1:0.1;len=-1:2:0.5" --out=weights.json

Model flags are train.py's (same parser and loading as transcribe.py).  Tuning flags:
  --ckpt, --vocab_path, --cmvn, --frontend, --resample, --batch_size, --manifest     as evaluate.py's
  --search         attention_beam (default) or ctc_prefix_beam
  --beam_size, --nbest     the search's beam and the entries kept per utterance (10, 10; at most 64 entries)
  --joint, --frame_topk, --blank_skip, --context, --context_score     forwarded to the search, as evaluate.py's
  --grid           name=values;name=values;...  One axis per column; the grid is their Cartesian product, row-major in the order given, at
                   most 65536 points and 8 columns.  values: lo:hi:step (both ends included, the points are lo + i * step in float64),
                   a,b,c or one number.  Columns: the scores the search reports (ctc_score, att_score, bias, lm_score, score), lm (the n-gram
                   LM score of the finished string; needs --lm) and len (the token count)
  --lm             the rescoring LM: an ARPA file (compiled with weight 1 and no insertion bonus, so the swept weight is the LM weight) or
                   an .npz saved from such an LM.  It is not forwarded to the search
  --out            a JSON file: the grid, the counts of every point, the best point and its weights (evaluate.py --rescore reads it)
Prints one JSON line per grid point {"g", "weights", "sub", "del", "ins", "cer", "ser"}, then one line {"best", "best_weights", "cer",
"rank0_cer", "oracle_cer", ...}.  The best point has the fewest errors; ties go to the fewest wrong utterances, then to the lowest index.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab  # noqa: E402
from asr_chinese_e2e_amd.data_handler.loader import parser_norm  # noqa: E402
from asr_chinese_e2e_amd.rescore import MAX_N, parse_grid  # noqa: E402
from evaluate import eval_options, manifest_batches, read_manifest, search_options  # noqa: E402
from train import TrainConfig, get_model_class, parse_flags  # noqa: E402
from transcribe import cmvn_path, load_model  # noqa: E402

CLI_KEYS = ("ckpt", "manifest", "search", "beam_size", "nbest", "joint", "blank_skip", "context", "context_score", "lm", "frame_topk", "out", "cmvn",
            "frontend", "resample", "batch_size", "grid")


def tune_options(cli):
    """The flags that can be judged before a model is loaded -> (search, num, grid); SystemExit for what is refused."""
    cli = dict(cli)
    cli.setdefault("search", "attention_beam")
    cli.setdefault("beam_size", 10)
    cli.setdefault("nbest", 10)
    search, num = eval_options({k: v for k, v in cli.items() if k in ("search", "beam_size", "nbest", "batch_size", "frame_topk")})
    if search == "transcribe":
        raise SystemExit("tune.py: --search must be attention_beam or ctc_prefix_beam (the weights re-rank an n-best list)")
    if num["nbest"] > MAX_N:
        raise SystemExit(f"tune.py: --nbest={num['nbest']}: lists of at most {MAX_N} entries are swept")
    if cli.get("grid") in (None, "", False, True):
        raise SystemExit("tune.py: give --grid=\"name=lo:hi:step;name=a,b,c;...\"")
    try:
        grid = parse_grid(str(cli["grid"]))
    except ValueError as e:
        raise SystemExit(f"tune.py: --grid: {e}") from e
    if "lm" in grid.names and cli.get("lm") in (None, "", False):
        raise SystemExit("tune.py: the grid has the column 'lm': give --lm=<ARPA file or .npz compiled with weight 1, ins 0>")
    return search, num, grid


def tune(**flags):
    cli = {k: flags.pop(k) for k in CLI_KEYS if k in flags}
    search, num, grid = tune_options(cli)
    entries = read_manifest(cli.get("manifest"))
    config = TrainConfig()
    config.fn_build(flags)
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(flags)
    if not torch.cuda.is_available():
        raise SystemExit("tune.py needs an MI355X: the searches and the sweep have no CPU fallback")
    vocab = Vocab.load(config.vocab_path)
    model = load_model(config, vocab, cli.get("ckpt"))
    parser = AudioParser(sample_rate=config.sample_rate, n_mels=config.n_mels, window_size=config.window_size,
                         lfr_m=config.lfr_m, lfr_n=config.lfr_n, frontend=str(cli.get("frontend", "reference")), **parser_norm(cmvn_path(cli)))
    lm = None
    path = cli.pop("lm", None)
    if path not in (None, "", False):
        from asr_chinese_e2e_amd.lm import NgramLM
        try:
            lm = NgramLM.load(str(path), device="cuda") if str(path).endswith(".npz") else NgramLM.from_arpa(str(path), vocab, weight=1.0, ins=0.0, device="cuda")
            lm.check_vocab(model.V)
        except (OSError, ValueError) as e:
            raise SystemExit(f"tune.py: --lm: {e}") from e
    kw = search_options(cli, model, vocab, search)
    batches = manifest_batches(entries, vocab, parser, num["batch_size"], config.sample_rate, bool(int(cli.get("resample", 0) or 0)))
    try:
        res = model.tune(batches, grid, search=search, beam_size=num["beam_size"], nbest=num["nbest"], lm=lm, **kw)
    except (ValueError, RuntimeError) as e:
        raise SystemExit(f"tune.py: {e}") from e
    report(res)
    if cli.get("out") not in (None, "", False):
        res.save(str(cli["out"]))
    return res


def report(res, file=None):
    """One line per grid point, then the best."""
    file = sys.stdout if file is None else file
    cer, ser = res.cer.tolist(), list(res.ser)
    for g in range(res.grid.shape[0]):
        line = {"g": g, "weights": dict(zip(res.names, res.grid[g].tolist())), "sub": int(res.sub[g]), "del": int(res.dele[g]), "ins": int(res.ins[g]),
                "cer": cer[g], "ser": float(ser[g])}
        print(json.dumps(line, ensure_ascii=False), file=file, flush=True)
    b = res.best
    print(json.dumps({"best": b, "best_weights": res.best_weights, "cer": cer[b], "ser": float(ser[b]), "rank0_cer": res.rank0_cer,
                      "oracle_cer": res.oracle_cer, "utterances": res.utterances, "ref_tokens": res.ref_tokens}, ensure_ascii=False), file=file, flush=True)


if __name__ == "__main__":
    tune(**parse_flags(sys.argv[1:]))
