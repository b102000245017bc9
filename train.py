#!/usr/bin/env python3
"""train.py - the reference's main.py (main.py:14-36, 38-41, 55-98) on the MI355X path.

    python train.py --model_name=TransformerOffical --batch_size=64 --warm_up=4000 --num_epoch=200 \
        --collector_path=data/collector --vocab_path=Predictor/vocab.t

Same flow: TrainConfig() <- fn_build(kwargs) ; ModelConfig merged over it (fn_combine) ; fn_build(kwargs) again ;
Vocab.load(vocab_path) ; build_dataloader(part = train / test / dev) ; Model(config, vocab).cuda() ;
Adam(lr=3e-4, betas=(0.9, 0.98), eps=1e-9) under NoamOpt(d_model, 1, warm_up) ; Trainer11(...).train().
Flags are `--key=value` pairs as fire would parse them (fire is not a dependency here); unknown keys are ADDED to the
config exactly as BaseConfig.fn_build does in the reference (base_config.py:7-15).

Differences that come with the MI355X path:
  * features are computed on the GPU per batch, so `predump` / `use_old` (cached .t feature files) are accepted and ignored;
  * multi-GPU: launch one process per GPU (python -m torch.distributed.run --nproc-per-node N train.py ...): the model is
    wrapped in dist.DataParallel (bucketed RCCL all-reduce overlapped with backward) and the loaders are sharded by rank -
    the reference's only multi-GPU hook is the commented-out `model.wrap()` (main.py:80);
  * `--speed_perturb=0.9,1.0,1.1` resamples every training utterance by one of these factors, drawn anew each epoch, on the GPU in
    front of the log-mel kernel (the reference has no waveform-side augmentation; dev and test are never perturbed);
  * `--noise_list=FILE --rir_list=FILE` (one wav path per line each) add noise and reverberation to the training utterances on the GPU,
    behind the speed perturbation: with probability `--rir_prob` (0.5) a room impulse response of the list is convolved in, with
    probability `--noise_prob` (0.5) a noise clip is mixed in at a signal-to-noise ratio drawn uniformly from `--snr_db=5,20` (dB);
    drawn anew each epoch, never for dev / test (the reference has no waveform-side augmentation); `--rir_method=direct|fft|auto` picks
    the reverberation kernel and `--rir_max_taps=N` the number of taps kept of a response (direct: at most 8192, the default; fft and
    auto: at most 65536, 4.1 s at 16 kHz);
  * `--cmvn=stats.npz` normalises the features of every part per mel bin with corpus statistics (tools/compute_cmvn.py) instead of
    per utterance: the causal features a streaming model is trained on (transcribe.py --stream=1 --cmvn=...);
  * `--frontend=kaldi` computes Kaldi fbank features (the front end of the Kaldi / WeNet / ESPnet / k2 recipes) instead of the
    reference's log-mel; statistics for `--cmvn` must then come from the same front end (tools/compute_cmvn.py --frontend=kaldi);
  * `--spec_aug=wenet` (`t2x50,f2x10`), `--spec_aug=espnet` (`w5,t2x40,f2x30`) or a policy of its own such as
    `--spec_aug=w5,t2x50,f2x10,s3x30,r200` masks, warps and substitutes the normalised frames of the train part on the GPU
    (data_handler/specaug.py; never dev / test, and instead of - not together with - the reference's `--augment`);
  * `--resample=1` accepts files at 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2 and 96 kHz (corpus, noise clips, responses) and converts
    them to 16 kHz on the GPU (data_handler/resample.py); without it a file at another rate raises, as before;
  * `--ema_decay=0.999` keeps an exponential moving average of the parameters inside the fused Adam pass (`--ema_warmup=False` switches
    the warm-up `min(decay, (1 + s) / (10 + s))` off); both are model-config keys and reach the model like every other one.  The trainers
    then write e{E}_s{S}.ema.model beside every checkpoint and log dev/ema/loss, dev/ema/cer beside the raw figures; average.py takes the
    mean of the last or best N checkpoints afterwards;
  * `--model_name=TransformerCTC --mwer_weight=0.5` fine-tunes on the expected number of errors over the model's own n-best list (MWER):
    the loss gains mwer_weight * the mean risk of the batch and the log gains `mwer`; `--mwer_nbest=4 --mwer_beam=4 --mwer_frame_topk=7
    --mwer_blank_skip=0.98` shape the device search that makes the list.  Model-config keys like ema_decay; 0 (the default) changes nothing;
  * `--model_name=TransformerCTC --cr_ctc_weight=0.2` trains with consistency regularisation (CR-CTC): the training loader yields two
    views of every utterance (views=2: 2 * batch_size rows, each view under its own draw of `--spec_aug`; the dev and test loaders stay
    at one view), the loss gains cr_ctc_weight * the mean consistency term between the two views' frame posteriors and the log gains
    `cr`.  A model-config key like mwer_weight, and not together with it; 0 (the default) changes nothing;
  * `--model_name=TransformerCTC --interctc_weight=0.3 --interctc_layers=3 --interctc_condition=1` trains with intermediate CTC: the
    shared CTC head is also applied to the output of the listed encoder layers (`--interctc_layers=2,4` lists two), the loss becomes
    (1 - w) CTC + w * the mean of their CTC losses and the log gains `interctc`; `--interctc_condition=1` adds self-conditioning (one more
    parameter, encoder.conditioning_layer.weight).  Model-config keys like mwer_weight, and not together with it or with cr_ctc_weight;
  * `--synthetic=N` trains on N synthetic AISHELL-1-shaped utterances (no dataset ships with this repository);
  * `--trainer=BaseTrainer` selects the twin of Trainer/base_trainer.py instead of Trainer11.
"""
import ast
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd import Models  # noqa: E402
from asr_chinese_e2e_amd.data_handler import DataConfigAiShell1, Vocab, build_dataloader, synthetic_pack  # noqa: E402
from asr_chinese_e2e_amd.Trainer import BaseTrainer, FusedAdam, NoamOpt, Trainer11  # noqa: E402


class TrainConfig(DataConfigAiShell1):      # main.py:14-36
    lr = 1e-3
    batch_size = 16
    eval_batch_size = 16
    num_epoch = 20
    warm_up = 1000
    device_id = [0, 1]
    exp_name = None
    drop_exp = True
    ckpt_root = "ckpt/"
    log_every_iter = 100
    eval_every_iter = 20000
    save_every_iter = 10000
    from_ckpt = None
    from_epoch = None
    from_step = None
    reference = "-loss"
    model_name = "TransformerOffical"      # the reference's class default is the stub 'ExampleModel'; its CLI default (main.py:103) is this
    predump = False
    use_old = False
    collector_path = "data/collector"       # data_config.py:18-19
    vocab_path = "Predictor/vocab.t"
    synthetic = 0                           # > 0: that many synthetic utterances instead of the manifests
    synthetic_frames = 500
    synthetic_vocab = 4232
    trainer = "Trainer11"
    cmvn = ""                               # --cmvn=stats.npz: global CMVN statistics for train, dev and test; empty = per-utterance normalisation
    frontend = "reference"                  # --frontend=kaldi: Kaldi fbank features (AudioParser(frontend="kaldi")) for train, dev and test
    noise_list = ""                         # --noise_list=FILE: wav paths of noise clips, one per line (train part only); empty = off
    rir_list = ""                           # --rir_list=FILE: wav paths of room impulse responses, one per line (train part only); empty = off
    noise_prob = 0.5                        # probability that an utterance gets noise / a response, drawn per epoch
    rir_prob = 0.5
    rir_method = "direct"                   # --rir_method=direct|fft|auto: the direct FIR kernel, the FFT overlap-save kernels, or chosen per bank
    rir_max_taps = 8192                     # --rir_max_taps=N: taps kept of a response (direct: at most 8192; fft / auto: at most 65536)
    snr_db = (5, 20)                        # --snr_db=5,20: the signal-to-noise ratio of a noisy utterance is uniform in this range (dB)
    resample = 0                            # --resample=1: files (corpus, noise, responses) at another rate than 16 kHz are converted on the GPU; 0 = they raise
    speed_perturb = ()                      # --speed_perturb=0.9,1.0,1.1: speed factors of the train part (never dev / test); empty = off
    spec_aug = ""                           # --spec_aug=wenet|espnet|w5,t2x50,f2x10,s3x30,r200: SpecAugment policy of the train part; empty = off


def get_model_class(model_name):            # main.py:38-41
    Model = getattr(Models, model_name)
    return Model, Model.get_default_config()


def parse_flags(argv):
    """--key=value / --key value / --flag  ->  dict with Python literals where they parse (as fire does)."""
    out, i = {}, 0
    while i < len(argv):
        a = argv[i]
        if not a.startswith("--"):
            raise SystemExit(f"unexpected argument {a!r} (flags are --key=value)")
        if "=" in a:
            k, v = a[2:].split("=", 1)
        elif i + 1 < len(argv) and not argv[i + 1].startswith("--"):
            k, v = a[2:], argv[i + 1]
            i += 1
        else:
            k, v = a[2:], "True"
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        out[k.replace("-", "_")] = v
        i += 1
    return out


def speed_factors(v):
    """The value of --speed_perturb as a tuple of factors, or None: `0.9,1.0,1.1` parses as a tuple, `0.9` as one number, anything else
    stays a comma-separated string."""
    if v is None or v is False or v == "" or v == ():
        return None
    if isinstance(v, str):
        return tuple(x.strip() for x in v.split(",") if x.strip()) or None
    return tuple(v) if isinstance(v, (tuple, list)) else (v,)


def path_list(v):
    """The value of --noise_list / --rir_list: the non-empty lines of that file, or None when the flag is empty."""
    if not v:
        return None
    with open(v, encoding="utf-8") as f:
        return [line.strip() for line in f if line.strip()]


def snr_range(v):
    """The value of --snr_db as (lo, hi): `5,20` parses as a tuple, `10` as one number (lo = hi)."""
    if isinstance(v, str):
        v = tuple(float(x) for x in v.split(",") if x.strip())
    v = tuple(float(x) for x in v) if isinstance(v, (tuple, list)) else (float(v),)
    if len(v) not in (1, 2) or v[0] > v[-1]:
        raise ValueError(f"--snr_db={v}: one number or lo,hi")
    return v[0], v[-1]


def loader_views(cr_ctc_weight):
    """--cr_ctc_weight > 0: the training loader yields two views of every utterance (the model checks the value itself)."""
    try:
        return 2 if float(cr_ctc_weight) > 0.0 else 1
    except (TypeError, ValueError):
        return 1


class _SyntheticLoader:
    """len(data) synthetic batches with the reference's batch contract, sharded by rank like the real loader."""

    def __init__(self, n_utt, batch, frames, feat, vocab, seed, rank, world, views=1):
        self.args = (batch, frames, feat, vocab)
        self.views = views      # 2: every batch twice over, [the B utterances | the same B] (the views then differ by dropout only)
        n = n_utt // batch
        self.seeds = [seed + i for i in range(n // world * world)][rank::world] if world > 1 else [seed + i for i in range(n)]

    def __len__(self):
        return len(self.seeds)

    def __iter__(self):
        B, T, F, V = self.args
        for s in self.seeds:
            pack = synthetic_pack(B, T, F, V, seed=s, ragged=True, device="cuda", dtype=torch.bfloat16)
            yield pack if self.views == 1 else type(pack)({k: torch.cat([v, v]) for k, v in pack.items()})


def train(**kwargs):                        # main.py:55-98
    print("\nStart training\n")
    config = TrainConfig()
    config.fn_build(kwargs)
    assert config.model_name
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(kwargs)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if rank == 0:
        config.fn_show()
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X: the training path has no CPU fallback")
    if world > 1:
        from asr_chinese_e2e_amd import dist as D
        D.init(os.environ.get("ASR_DIST_BACKEND", "nccl"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    views = loader_views(getattr(config, "cr_ctc_weight", 0.0))
    if config.synthetic:
        vocab = Vocab.synthetic(config.synthetic_vocab)
        F = config.n_mels * config.lfr_m
        mk = lambda n, b, seed, views=1: _SyntheticLoader(n, b, config.synthetic_frames, F, vocab.vocab_size, seed, rank, world, views)
        train_iter = mk(config.synthetic, config.batch_size, 1000, views)
        test_iter = mk(max(config.synthetic // 8, config.eval_batch_size), config.eval_batch_size, 5000)
        dev_iter = mk(max(config.synthetic // 8, config.eval_batch_size), config.eval_batch_size, 7000)
    else:
        vocab = Vocab.load(config.vocab_path)
        common = dict(collector_path=config.collector_path, vocab=vocab, sample_rate=config.sample_rate, window_size=config.window_size,
                      n_mels=config.n_mels, predump=config.predump, use_old=config.use_old, lfr_m=config.lfr_m, lfr_n=config.lfr_n,
                      rank=rank, world=world, cmvn=config.cmvn or None, resample=bool(int(config.resample)), frontend=str(config.frontend))
        train_iter = build_dataloader(batch_size=config.batch_size, part="train", augment=config.augment, speed_perturb=speed_factors(config.speed_perturb),
                                      noise=path_list(config.noise_list), rir=path_list(config.rir_list), noise_prob=float(config.noise_prob),
                                      rir_prob=float(config.rir_prob), snr_db=snr_range(config.snr_db), rir_method=str(config.rir_method),
                                      rir_max_taps=int(config.rir_max_taps), spec_augment=str(config.spec_aug or "") or None, views=views, **common)
        test_iter = build_dataloader(batch_size=config.eval_batch_size, part="test", augment=False, **common)
        dev_iter = build_dataloader(batch_size=config.eval_batch_size, part="dev", augment=False, **common)

    model = Model(config, vocab).cuda()
    optimizer = FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-09)      # main.py:81
    assert config.hidden_size
    optimizer = NoamOpt(config.d_model, 1, config.warm_up, optimizer)                      # main.py:83
    runner = model
    if world > 1:
        runner = D.DataParallel(model, torch.device("cuda", torch.cuda.current_device()))
    Trainer = {"Trainer11": Trainer11, "BaseTrainer": BaseTrainer}[config.trainer]
    exp_name = config.exp_name if world == 1 or config.exp_name is None else f"{config.exp_name}"
    trainer = Trainer(model=runner, optimizer=optimizer, train_iter=train_iter, dev_iter=dev_iter, test_iter=test_iter, exp_name=exp_name,
                      ckpt_root=config.ckpt_root if rank == 0 else os.path.join(config.ckpt_root, f"rank{rank}"),
                      eval_every_iter=config.eval_every_iter, log_every_iter=config.log_every_iter, save_every_iter=config.save_every_iter,
                      drop_exp=config.drop_exp)
    print(f"start trainning at {trainer.get_time()}\n")
    if config.from_ckpt is not None:
        if config.trainer == "BaseTrainer":
            trainer.train((config.from_ckpt, config.from_epoch, config.from_step))
        else:
            trainer.train(config.from_ckpt, config.from_epoch, config.from_step)
    else:
        trainer.train()
    print(f"done at {trainer.get_time()}\n")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return trainer


if __name__ == "__main__":
    train(**parse_flags(sys.argv[1:]))
