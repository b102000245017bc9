"""TransformerOffical / TransformerCTC: the reference's model plugin surface on the HIP engine.

Mirrors Predictor/Models/transformer_official.py:34-125 of the reference:
    Model(config, vocab); .cuda(); .parameters(); .state_dict() with the SAME key names;
    .iterate(pack, optimizer=..., is_train=...) -> (metrics Pack{loss, cer}, None);
    .forward(pack) -> Pack{pred, gold}; .cal_metrics(output, pack); .get_default_config()
so the reference's main.py / Trainer11 drive it unchanged.  What runs underneath is the explicit
forward/backward engine (engine.py) on hand-written HIP kernels - there is no autograd graph
and NO CPU fallback: iterate() on CPU tensors raises.

Additions required by BASELINE.json's north_star (not in the reference):
  * config.ctc_weight = lambda in [0,1]: joint loss lambda*CTC + (1-lambda)*CE via a `ctc_lo`
    head on the encoder output (lambda = 0 reproduces the reference exactly),
  * TransformerCTC: encoder + CTC only (BASELINE config 2),
  * config.cross_mask: "ref_compat" reproduces the reference's decoder cross-attention mask built
    from TEXT lengths (transformer_official.py:78, 301-303); "wave_len" is the corrected mask,
  * config.dtype: "bf16" (default) or "fp32" (exact-fp32 parity mode),
  * config.attn_window: +-w frame band on encoder self-attention (long-form config), -1 = full,
  * config.chunk_size / left_chunks / decoding_chunk_size / decoding_left_chunks: chunk-masked encoder self-attention for
    streaming (WeNet U2's subsequent_chunk_mask; encoder_mask() below), and model.stream() (stream.py),
  * config.ema_decay in [0, 1) / ema_warmup: an exponential moving average of the parameters kept beside them in the flat buffers and
    updated inside the fused Adam pass (include/asr_hip.h: asr_adam_ema_step); ema_state_dict() / save_ema() / load_ema() / ema_weights().
    0 (the default) allocates nothing and launches what was launched without it.
  * config.mwer_weight > 0 (TransformerCTC only) / mwer_nbest / mwer_beam / mwer_frame_topk / mwer_blank_skip: MWER training - the step's
    loss gains mwer_weight * the mean over the batch of the expected number of errors over the model's own n-best list (the device
    prefix beam search on the step's logits; include/asr_hip.h: asr_ctc_mwer_lattice, engine.ctc_fwd_bwd), metrics gains `mwer`;
    model.mwer_risk(pack) reports the same figures without a gradient.  0 (the default) launches what was launched without it.
  * config.cr_ctc_weight > 0 (TransformerCTC only): CR-CTC training - the batch holds two views of every utterance (rows p and p + B/2,
    data_handler.BucketedWaveLoader(views=2)) and the step's loss gains cr_ctc_weight * the mean over the pairs of the consistency term
    between the two views' frame posteriors (include/asr_hip.h: asr_cr_ctc_fwd_bwd, engine.ctc_fwd_bwd), metrics gains `cr`.
    0 (the default) launches what was launched without it.
  * config.interctc_weight = w in (0, 1) with config.interctc_layers (TransformerCTC only): intermediate CTC - the shared CTC head is
    also applied to the output of the listed encoder layers and the loss becomes (1 - w) CTC + w * the mean of their CTC losses;
    config.interctc_condition adds self-conditioning: the layers' frame posteriors, projected back to d_model by
    encoder.conditioning_layer.weight (d_model, V; no bias), are added to the next layer's input - in training and in inference
    (include/asr_hip.h: asr_softmax_rows, asr_softmax_bwd_add; engine.encoder_fwd / encoder_bwd; the definition is
    tests/interctc_ref.py).  metrics gains `interctc`; model.interctc_losses(pack) reports the losses without a gradient.  The defaults
    launch what was launched without them and add no parameter.
"""
import contextlib
import math

import numpy as np
import torch

from .. import engine as E
from .. import kernels as K
from ..Bases import BaseConfig, BaseModel
from ..Utils import Pack

SOS_ID, EOS_ID, PAD_ID = 2, 3, 0   # transformer_official.py:53-54, Utils/loss.py:5
PE_MAXLEN = 5000                   # transformer_official.py:49, 65
CLIP_NORM = 5.0                    # transformer_official.py:102


def mwer_settings(weight, nbest, beam, frame_topk, blank_skip):
    """The MWER keys as the engine takes them: (weight, dict(nbest, beam, frame_topk, thr)); ValueError for what the device search or the
    lattice kernels would refuse - before anything is launched."""
    try:
        ok = not isinstance(weight, (bool, str)) and math.isfinite(float(weight)) and float(weight) >= 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"mwer_weight={weight!r}: a finite number >= 0 (0 = no MWER term)")
    for name, v in (("mwer_nbest", nbest), ("mwer_beam", beam), ("mwer_frame_topk", frame_topk)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}={v!r}: an integer")
    nbest, beam, frame_topk = int(nbest), int(beam), int(frame_topk)
    if beam < 2 or beam > K.MWER_MAX_N or not 2 <= nbest <= beam:
        raise ValueError(f"mwer_nbest={nbest} must lie in [2, mwer_beam] and mwer_beam={beam} in [2, {K.MWER_MAX_N}]")
    if frame_topk < 1 or beam * (frame_topk + 1) > 64:
        raise ValueError(f"the device search ranks mwer_beam * (mwer_frame_topk + 1) <= 64 candidates per frame (beam {beam}, frame_topk {frame_topk})")
    thr = None if blank_skip is None else K.blank_skip_threshold(blank_skip)
    return float(weight), dict(nbest=nbest, beam=beam, frame_topk=frame_topk, thr=thr)


def cr_ctc_setting(weight):
    """config.cr_ctc_weight as a float; ValueError unless it is a finite number >= 0."""
    try:
        ok = not isinstance(weight, (bool, str)) and math.isfinite(float(weight)) and float(weight) >= 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"cr_ctc_weight={weight!r}: a finite number >= 0 (0 = no consistency term)")
    return float(weight)


def interctc_settings(weight, layers, condition, layer_num):
    """(w, layers, condition) of config.interctc_weight / interctc_layers / interctc_condition for an encoder of layer_num layers;
    ValueError unless w is a finite number in [0, 1), the layers - a tuple or list of ints, or a string like "3" or "2,4" - are strictly
    increasing 1-based encoder layers in [1, layer_num - 1], w > 0 exactly when layers are listed, and conditioning comes with layers."""
    try:
        ok = not isinstance(weight, (bool, str)) and math.isfinite(float(weight)) and 0.0 <= float(weight) < 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"interctc_weight={weight!r}: a finite number in [0, 1) (0 = no intermediate CTC)")
    w = float(weight)
    raw = layers
    try:
        if isinstance(layers, str):
            layers = [int(t) for t in layers.split(",")] if layers.strip() else []
        elif isinstance(layers, (tuple, list)):
            if any(isinstance(l, bool) or not isinstance(l, (int, np.integer)) for l in layers):
                raise ValueError
            layers = [int(l) for l in layers]
        elif isinstance(layers, (int, np.integer)) and not isinstance(layers, bool):      # --interctc_layers=3 parses as a number
            layers = [int(layers)]
        elif layers is None:
            layers = []
        else:
            raise ValueError
    except ValueError:
        raise ValueError(f"interctc_layers={raw!r}: a tuple or list of encoder layers, or a string like '3' or '2,4'") from None
    if any(l < 1 or l > layer_num - 1 for l in layers) or any(a >= b for a, b in zip(layers, layers[1:])):
        raise ValueError(f"interctc_layers={raw!r}: strictly increasing 1-based encoder layers in [1, {layer_num - 1}] (layer_num = {layer_num})")
    if not isinstance(condition, (bool, int, np.integer)) or condition not in (0, 1):
        raise ValueError(f"interctc_condition={condition!r}: True or False")
    if (w > 0.0) != bool(layers):
        raise ValueError(f"interctc_weight={w} with interctc_layers={tuple(layers)}: a weight > 0 needs layers, and layers need a weight > 0")
    if condition and not layers:
        raise ValueError("interctc_condition needs interctc_layers")
    return w, tuple(layers), bool(condition)


def _set_nested(root, dotted, value, is_buffer=False):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, torch.nn.Module())
        mod = getattr(mod, p)
    if is_buffer:
        mod.register_buffer(parts[-1], value)
    else:
        mod.register_parameter(parts[-1], value)


class _SpeechTransformer(BaseModel):
    USE_DECODER = True

    def __init__(self, config, vocab):
        super().__init__()
        self.config = config
        self.vocab = vocab
        c = config
        self.use_decoder = self.USE_DECODER
        lam = float(getattr(c, "ctc_weight", 0.0))
        self.ctc_weight = lam if self.use_decoder else 1.0
        self.use_ctc = (lam > 0.0) or not self.use_decoder
        self.cross_mask = getattr(c, "cross_mask", "ref_compat")
        self.lowp = str(getattr(c, "dtype", "bf16")).lower() in ("bf16", "bfloat16")
        self.attn_window = int(getattr(c, "attn_window", -1))
        self.chunk_size = int(getattr(c, "chunk_size", 0))
        self.left_chunks = int(getattr(c, "left_chunks", -1))
        dcs, dlc = getattr(c, "decoding_chunk_size", None), getattr(c, "decoding_left_chunks", None)
        static = self.chunk_size > 0
        self.decoding_chunk_size = int(dcs) if dcs is not None else (self.chunk_size if static else 0)
        self.decoding_left_chunks = int(dlc) if dlc is not None else (self.left_chunks if static else -1)
        if self.chunk_size < -1 or self.left_chunks < -1 or self.decoding_chunk_size < 0 or self.decoding_left_chunks < -1:
            raise ValueError(f"bad chunk configuration: chunk_size={self.chunk_size} left_chunks={self.left_chunks} "
                             f"decoding_chunk_size={self.decoding_chunk_size} decoding_left_chunks={self.decoding_left_chunks}")
        if (self.chunk_size != 0 or self.decoding_chunk_size > 0) and self.attn_window >= 0:
            raise ValueError("a chunk mask (chunk_size / decoding_chunk_size) and attn_window are mutually exclusive")
        self._enc_given = None      # (enc, B, T): an encoder output the inference paths take instead of running the encoder (stream.py)
        self.label_smoothing = float(getattr(c, "label_smoothing", 0.0))   # Utils/loss.py:30-45 (the reference never enables it)
        self.cer_in_iterate = bool(getattr(c, "cer_in_iterate", True))
        self._step_seed = int(getattr(c, "seed", 0))   # advanced once per training step (dropout masks)
        decay = getattr(c, "ema_decay", 0.0)
        try:
            ok = not isinstance(decay, (bool, str)) and math.isfinite(float(decay)) and 0.0 <= float(np.float32(decay)) < 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:      # as the kernel takes it: a float32 inside (0, 1), or 0 = off
            raise ValueError(f"ema_decay={decay!r}: a finite number in [0, 1) (0 = no average)")
        self.ema_decay = float(decay)
        self.ema_warmup = bool(getattr(c, "ema_warmup", True))
        self._ema_step = 0           # steps counted here for optimizers that keep no _step of their own
        self._ema_active = False     # inside ema_weights(): p holds the average, ema the raw parameters
        self._ema_pending = None     # an average loaded (load_ema) before the flat buffers existed
        self.mwer_weight, self._mwer = mwer_settings(getattr(c, "mwer_weight", 0.0), getattr(c, "mwer_nbest", 4), getattr(c, "mwer_beam", 4),
                                                     getattr(c, "mwer_frame_topk", 7), getattr(c, "mwer_blank_skip", None))
        self._mwer_mean = None       # the mean risk of the last training step (device scalar), None without the MWER term
        if self.mwer_weight > 0.0 and self.use_decoder:
            raise ValueError("mwer_weight > 0 needs the CTC-only model (TransformerCTC): MWER through the attention decoder is not implemented")
        self.cr_ctc_weight = cr_ctc_setting(getattr(c, "cr_ctc_weight", 0.0))
        self._cr_mean = None         # the mean consistency term of the last training step's pairs (device scalar), None without the term
        if self.cr_ctc_weight > 0.0 and self.use_decoder:
            raise ValueError("cr_ctc_weight > 0 needs the CTC-only model (TransformerCTC): the consistency term is defined on the CTC head's posteriors")
        if self.cr_ctc_weight > 0.0 and self.mwer_weight > 0.0:
            raise ValueError("cr_ctc_weight > 0 together with mwer_weight > 0 is not implemented: both add a gradient on top of the CTC gradient")
        self.interctc_weight, self.interctc_layers, self.interctc_condition = interctc_settings(
            getattr(c, "interctc_weight", 0.0), getattr(c, "interctc_layers", ()), getattr(c, "interctc_condition", False), int(c.layer_num))
        self._interctc_mean = None   # the mean intermediate CTC loss of the last training step (device scalar), None without the term
        if self.interctc_layers and self.use_decoder:
            raise ValueError("interctc_weight > 0 needs the CTC-only model (TransformerCTC): intermediate CTC for the joint model is not implemented")
        if self.interctc_layers and (self.mwer_weight > 0.0 or self.cr_ctc_weight > 0.0):
            raise ValueError("interctc_weight > 0 together with mwer_weight > 0 or cr_ctc_weight > 0 is not implemented")
        d, H, dk, ff = c.d_model, c.num_head, c.hidden_size, c.ff_size
        d_in = c.n_mels * c.lfr_m
        V = vocab.vocab_size
        self.V = V

        # ---- parameter blocks in FORWARD order (backward finishes them in reverse: dist.py)
        blocks = [[("encoder.linear_in.weight", (d, d_in))], [("encoder.linear_in.bias", (d,))],
                  [("encoder.layer_norm_in.weight", (d,))], [("encoder.layer_norm_in.bias", (d,))]]
        for i in range(c.layer_num):
            blocks += E.mha_param_block(f"encoder.layer_stack.{i}.slf_attn.", H, dk, d)
            blocks += E.ffn_param_block(f"encoder.layer_stack.{i}.pos_ffn.", d, ff)
        if self.interctc_condition:      # directly in front of the head: both become final at the same point of the backward pass
            blocks += [[(E.COND_NAME, (d, V))]]
        if self.use_ctc:
            blocks += [[("ctc_lo.weight", (V, d))], [("ctc_lo.bias", (V,))]]
        if self.use_decoder:
            blocks += [[("decoder.tgt_word_emb.weight", (V, d))]]
            # the cross-attention K | V projections of ALL decoder layers side by side: they all multiply the same encoder output
            # (transformer_official.py:309-314, 446-458), so the six projections are one (L 2 H dk, d) matrix to the engine
            blocks += E.cross_kv_param_blocks([f"decoder.layer_stack.{i}.enc_attn." for i in range(c.layer_num)], H, dk, d)
            for i in range(c.layer_num):
                blocks += E.mha_param_block(f"decoder.layer_stack.{i}.slf_attn.", H, dk, d)
                blocks += E.cross_q_param_block(f"decoder.layer_stack.{i}.enc_attn.", H, dk, d)
                blocks += E.ffn_param_block(f"decoder.layer_stack.{i}.pos_ffn.", d, ff)
        self._flat = E.FlatParams(blocks)
        self._engine = None
        self._views_checked = False   # parameters verified to be views of the flat buffer
        self._grads_checked = False   # .grad attributes verified to be views of the flat gradient
        self._flat_device = None

        # ---- nn.Parameters with the reference's names / shapes / init distributions
        order = self._state_order(c.layer_num)
        for name in order:
            if name.endswith("positional_encoding.pe"):
                _set_nested(self, name, E.positional_encoding(PE_MAXLEN, d), is_buffer=True)
            elif name == "decoder.tgt_word_prj.weight":
                _set_nested(self, name, self.decoder.tgt_word_emb.weight)   # tied (transformer_official.py:253-256)
            else:
                wname = name[:-5] + ".weight" if name.endswith(".bias") else name
                wshape = self._flat.index[wname][1]
                _set_nested(self, name, torch.nn.Parameter(self._init_tensor(name, self._flat.index[name][1], wshape, d, dk)))

    # state_dict key order of the reference (module registration order)
    def _state_order(self, L):
        def mha(pre):
            return [pre + n for n in ("w_qs.weight", "w_qs.bias", "w_ks.weight", "w_ks.bias", "w_vs.weight", "w_vs.bias",
                                      "layer_norm.weight", "layer_norm.bias", "fc.weight", "fc.bias")]

        def ffn(pre):
            return [pre + n for n in ("w_1.weight", "w_1.bias", "w_2.weight", "w_2.bias", "layer_norm.weight", "layer_norm.bias")]

        names = ["encoder.linear_in.weight", "encoder.linear_in.bias", "encoder.layer_norm_in.weight",
                 "encoder.layer_norm_in.bias", "encoder.positional_encoding.pe"]
        for i in range(L):
            names += mha(f"encoder.layer_stack.{i}.slf_attn.") + ffn(f"encoder.layer_stack.{i}.pos_ffn.")
        if self.interctc_condition:
            names += [E.COND_NAME]
        if self.use_decoder:
            names += ["decoder.tgt_word_emb.weight", "decoder.positional_encoding.pe"]
            for i in range(L):
                names += mha(f"decoder.layer_stack.{i}.slf_attn.") + mha(f"decoder.layer_stack.{i}.enc_attn.") + ffn(f"decoder.layer_stack.{i}.pos_ffn.")
            names += ["decoder.tgt_word_prj.weight"]
        if self.use_ctc:
            names += ["ctc_lo.weight", "ctc_lo.bias"]
        return names

    @staticmethod
    def _init_tensor(name, shape, wshape, d, dk):
        """attention.py:16-28, transformer_official.py:147-156, 242-256, torch defaults elsewhere."""
        t = torch.empty(*shape)
        leaf = name.rsplit(".", 2)[-2]
        if leaf in ("layer_norm", "layer_norm_in"):
            return t.fill_(1.0) if name.endswith(".weight") else t.zero_()
        fan_out, fan_in = wshape[0], wshape[1]
        if name == "decoder.tgt_word_emb.weight":
            return t.normal_(0.0, 1.0)            # nn.Embedding default; the tied projection reuses it
        if name.endswith(".weight"):
            if leaf in ("w_qs", "w_ks", "w_vs"):
                return t.normal_(0.0, math.sqrt(2.0 / (d + dk)))
            if leaf in ("fc", "linear_in", "ctc_lo", "conditioning_layer"):
                return t.normal_(0.0, math.sqrt(2.0 / (fan_in + fan_out)))   # xavier_normal_
        bound = 1.0 / math.sqrt(fan_in)            # Linear / Conv1d default: U(+-1/sqrt(fan_in)), weights and biases
        return t.uniform_(-bound, bound)

    # ------------------------------------------------------------------ flat storage management
    def _named_flat_params(self):
        for name, p in self.named_parameters():
            yield name, p

    def _ensure_engine(self, device):
        """(Re)build the flat HBM buffers when the parameters are not views of them (first call,
        after .cuda()/.to(), after load_state_dict on a fresh module)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:   # "cuda" and "cuda:0" must compare equal below
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise RuntimeError("the HIP engine runs on an MI355X only: move the model and batch to 'cuda' "
                               "(there is no CPU fallback; the CPU oracle lives in oracle/ for tests)")
        f = self._flat
        ok = self._engine is not None and self._flat_device == device
        if ok and self._views_checked:      # fast path of every step: nothing has touched the parameters' storage
            return self._engine
        if ok:
            for name, p in self._named_flat_params():
                off, shape = f.index[name]
                if p.data_ptr() != f.p.data_ptr() + 4 * off:
                    ok = False
                    break
        if ok:
            self._views_checked = True
            return self._engine
        K.bind_device(device)
        old = {name: p.detach().to(device=device, dtype=torch.float32) for name, p in self._named_flat_params()}
        old_mv = (f.m.to(device), f.v.to(device)) if f.m is not None else None   # keep Adam state across a device move
        old_ema = f.ema.to(device) if f.ema is not None else None                # ... and the average
        f.allocate(device, self.lowp, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        if old_mv is not None:
            f.m.copy_(old_mv[0])
            f.v.copy_(old_mv[1])
        for name, p in self._named_flat_params():
            view = f.view(f.p, name)
            view.copy_(old[name].view(view.shape))
            p.data = view
            p.grad = f.view(f.g, name)
        if f.ema is not None:
            f.ema.copy_(f.p if old_ema is None else old_ema)      # a new average starts as a copy of p (the gaps between blocks: zero, as in p)
            if self._ema_pending is not None:
                self._fill_ema(self._ema_pending)
                self._ema_pending = None
        f.refresh_lowp()
        for b in self.buffers():
            b.data = b.data.to(device)
        pe = self.encoder.positional_encoding.pe[0].to(device).contiguous()
        self._engine = E.Engine(f, self.config, self.V, self.use_decoder, self.use_ctc, pe)
        self._engine.mwer = dict(self._mwer) if self.mwer_weight > 0.0 else None
        self._engine.cr_ctc = self.cr_ctc_weight > 0.0
        self._engine.interctc = (self.interctc_layers, self.interctc_weight, self.interctc_condition)
        self._flat_device = device
        self._views_checked = True
        self._grads_checked = True
        return self._engine

    def zero_grad(self, set_to_none=True):
        self._grads_checked = False      # nn.Module.zero_grad may drop the .grad views
        return super().zero_grad(set_to_none=set_to_none)

    def _apply(self, fn, *a, **kw):
        # .cuda() / .to() / .float() replace the parameters' storage: re-validate the flat views on the next step
        self._views_checked = False
        self._grads_checked = False
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, state_dict, strict=True, **kw):
        state_dict = {k: v for k, v in state_dict.items()}
        self._views_checked = False
        if self._ema_active:
            raise RuntimeError("load_state_dict inside ema_weights(): the parameters are swapped with their average")
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if self._flat.p is not None:
            self._flat.refresh_lowp()
        self._ema_pending = None
        f = self._flat
        if f.ema is not None:      # the average restarts from the loaded weights (load_ema overrides it)
            if all(p.data_ptr() == f.p.data_ptr() + 4 * f.index[n][0] for n, p in self._named_flat_params()):
                f.ema.copy_(f.p)
            else:                  # the parameters left the flat buffer: _ensure_engine rebuilds it, and the average from p
                f.ema = None
        return out

    # ------------------------------------------------------------------ the average of the parameters (config.ema_decay > 0)
    def _need_ema(self, what):
        if self.ema_decay <= 0:
            raise RuntimeError(f"{what}: the model keeps no average (config.ema_decay is 0)")

    def _fill_ema(self, state):
        """Write a state dict with the model's keys into the flat average (every parameter key must be there)."""
        f = self._flat
        names = [n for n, _ in self._named_flat_params()]
        missing = [n for n in names if n not in state]
        if missing:
            raise KeyError(f"the average lacks {len(missing)} parameters of the model: {missing[:5]}")
        for n in names:
            view = f.view(f.ema, n)
            if tuple(state[n].shape) != tuple(view.shape):
                raise ValueError(f"the average's {n} has shape {tuple(state[n].shape)}, the model {tuple(view.shape)}")
            view.copy_(state[n])

    def ema_state_dict(self):
        """The average as a plain state dict with the model's keys (buffers included, on the CPU): it loads into a model of this package
        built with or without an average, and into the reference's."""
        self._need_ema("ema_state_dict")
        f = self._flat
        if f.ema is None and self._ema_pending is not None:
            return {k: v.detach().cpu().clone() for k, v in self._ema_pending.items()}
        by_id = {id(p): n for n, p in self._named_flat_params()}
        src = f.p if self._ema_active else f.ema
        out = {}
        for k, v in self.state_dict(keep_vars=True).items():
            n = by_id.get(id(v))
            if n is not None and src is not None:
                out[k] = f.view(src, n).detach().cpu().clone()
            else:                                    # buffers; before the flat buffers exist the average is the parameters themselves
                out[k] = v.detach().cpu().clone()
        return out

    def save_ema(self, path):
        torch.save(self.ema_state_dict(), path)
        print(f"\nmodel average saved to {path}")

    def load_ema(self, path):
        """Override the average with a file written by save_ema (after load / load_state_dict, which reset it to the weights).  A missing
        file or missing keys raise."""
        self._need_ema("load_ema")
        if self._ema_active:
            raise RuntimeError("load_ema inside ema_weights(): the parameters are swapped with their average")
        state = torch.load(path, map_location="cpu", weights_only=True)
        missing = [n for n, _ in self._named_flat_params() if n not in state]
        if missing:
            raise KeyError(f"{path} lacks {len(missing)} parameters of the model: {missing[:5]}")
        if self._flat.ema is None:
            self._ema_pending = state                # the flat buffers do not exist yet: _ensure_engine applies it
        else:
            self._fill_ema(state)
        print(f"\nLoaded model average from '{path}'")

    def _swap_ema(self):
        f = self._flat
        tmp = f.p.clone()
        f.p.copy_(f.ema)
        f.ema.copy_(tmp)
        f.refresh_lowp()
        f.version += 1

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters ARE the average (p and ema swapped, bf16 shadow refreshed): forward, transcribe, evaluate, the
        searches and stream run on it.  On exit they are swapped back.  Training inside the block raises."""
        self._need_ema("ema_weights")
        if self._ema_active:
            raise RuntimeError("ema_weights() is already active")
        self._ensure_engine(next(self.parameters()).device)
        self._swap_ema()
        self._ema_active = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_active = False

    def _ema_after_step(self, optimizer):
        """The average after a step of an optimizer that did not run the fused Adam + EMA pass: asr_ema_update with the optimizer's step
        count where it keeps one (NoamOpt._step), else a count kept here."""
        self._ema_step += 1
        s = getattr(optimizer, "_step", None)
        s = int(s) if isinstance(s, int) and not isinstance(s, bool) and s >= 1 else self._ema_step
        K.ema_update(self._flat.p, self._flat.ema, self.ema_decay, s, self.ema_warmup)

    def zero_flat_grads(self):
        """Zero the flat gradient buffer for the step that follows.  With the multi-stream engine the fill (160 MB at the joint model's size,
        ~20 us) is not queued in front of the forward pass on the main stream: train_step hands it to the weight-gradient stream - idle during
        the forward pass - in front of the transposed weight copies, whose event every backward path waits for before its first gradient write."""
        f = self._flat
        eng = self._engine
        self._zero_lazy = eng is not None and eng._tr_tiles is not None and eng.overlap_wgrad
        if not self._zero_lazy:
            f.g.zero_()
        if self._grads_checked:             # fast path: .grad views were verified and nobody reset them
            return
        for name, p in self._named_flat_params():
            if p.grad is None or p.grad.data_ptr() != f.g.data_ptr() + 4 * f.index[name][0]:
                p.grad = f.view(f.g, name)
        self._grads_checked = True

    # ------------------------------------------------------------------ reference API
    def _prepare(self, input, training=False):
        wave = input.wave
        eng = self._ensure_engine(wave.device)
        eng.training = bool(training)
        if training:
            self._step_seed = (self._step_seed + 1) & 0x7FFFFFFF
            eng.step_seed = self._step_seed
        x = wave if wave.dtype == eng.dtype else wave.to(eng.dtype)
        x = x.contiguous()
        if input.tgt_for_input is None:      # audio-only batch (inference): no label preprocessing, no decoder pass in forward()
            self._tgt_len32 = None
            return eng, x, self._len32_of(input.wave_len, (), ()).contiguous(), None
        tgt = input.tgt_for_input.contiguous()
        tl = input.tgt_len
        if self.cross_mask == "ref_compat" and tl is not None and tl.device.type == "cpu" and tl.numel() and int(tl.max()) > tgt.shape[1]:
            # the cross-attention's key rows are cut at the padded target width (Engine.cross_rows): a longer text length would see frames
            # that were never projected
            raise ValueError(f"tgt_len {int(tl.max())} exceeds the padded target width {tgt.shape[1]} of tgt_for_input")
        # the batch contract hands lengths over as int64 (ai_shell_1.py:75-88): the label preprocessing launch also makes the int32 copies
        lens64 = [t.contiguous() for t in (input.wave_len, input.tgt_len) if t is not None and t.dtype == torch.int64 and t.device == tgt.device]
        out = K.dec_preprocess(tgt, SOS_ID, EOS_ID, lens64=lens64)
        prep, lens32 = out[:6], (out[6] if lens64 else ())
        wave_len = self._len32_of(input.wave_len, lens64, lens32)
        self._tgt_len32 = self._len32_of(input.tgt_len, lens64, lens32) if input.tgt_len is not None else None
        return eng, x, wave_len, prep

    def _cross(self, eng, input, wave_len, T):
        """(key lengths, key rows Tk) of the decoder's encoder-decoder attention."""
        if self.cross_mask == "ref_compat":
            return self._tgt_len32, eng.cross_rows(input.tgt_for_input.shape[1], T, self._tgt_len32 is not None)
        return wave_len, T

    @staticmethod
    def _len32_of(t, lens64, lens32):
        """int32 copy of a length vector: the one dec_preprocess made when the vector went through it, else a cast."""
        for a, b in zip(lens64, lens32):
            if a.data_ptr() == t.data_ptr() and a.numel() == t.numel():
                return b
        return t.to(torch.int32)

    # ------------------------------------------------------------------ encoder mask (every encoder_fwd caller goes through here)
    DYN_CHUNK_MAX = 25      # dynamic chunk training: C uniform in [1, 25] (WeNet's dynamic-chunk recipe), full attention half the time

    @staticmethod
    def dynamic_chunk(step):
        """chunk_size = -1: the chunk of training step `step` (0 = full attention) - a pure function of the step counter, so it is the
        same on every data-parallel rank and on a replay."""
        x = (int(step) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF      # integer hash (murmur3 finaliser)
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        return 0 if (x & 1) == 0 else 1 + (x >> 1) % _SpeechTransformer.DYN_CHUNK_MAX

    def encoder_mask(self, training=False):
        """(chunk, left_chunks) of the encoder's self-attention: the training mask (chunk_size; -1 = this step's dynamic_chunk) or the
        decoding mask of every inference path.  (0, -1) = full attention (or the attn_window band)."""
        if training:
            C = self.dynamic_chunk(self._step_seed) if self.chunk_size == -1 else self.chunk_size
            return (C, self.left_chunks) if C > 0 else (0, -1)
        return (self.decoding_chunk_size, self.decoding_left_chunks) if self.decoding_chunk_size > 0 else (0, -1)

    def encode(self, eng, x, wave_len, training=False, interctc=None):
        """Engine.encoder_fwd under encoder_mask(training): (enc (B*T, d), cache).  Inside given_encoder_output() the inference paths get
        that output instead (cache None).  interctc: the labels and gradient scales of a step with intermediate CTC (Engine.encoder_fwd)."""
        if self._enc_given is not None and not training:
            enc, B, T = self._enc_given
            if x.shape[0] != B or x.shape[1] != T:
                raise ValueError(f"the given encoder output is for (B, T) = ({B}, {T}), the batch has {tuple(x.shape[:2])}")
            return enc, None
        chunk, left = self.encoder_mask(training)
        return eng.encoder_fwd(x, wave_len, self.attn_window, chunk, left, interctc=interctc)

    def given_encoder_output(self, enc):
        """Context manager: the searches (forward, ctc_greedy_search, ctc_prefix_beam_search, beam_search, transcribe) use `enc`
        ((B, T, d) in the model's dtype) as the encoder output of a batch of the same (B, T) instead of running the encoder."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            B, T = enc.shape[0], enc.shape[1]
            prev, self._enc_given = self._enc_given, (enc.reshape(B * T, -1).contiguous(), B, T)
            try:
                yield self
            finally:
                self._enc_given = prev
        return ctx()

    def stream(self, batch_size, parser=None, source_rate=None, search="greedy", beam_size=5, frame_topk=10, context=None, context_ids=None, lm=None,
               timed=False, confidence="post_max", beam_times=False, blank_skip=None, keywords=None):
        """A streaming encoder for `batch_size` utterances in lock-step (stream.StreamingEncoder, a view of sessions.Sessions with every
        slot opened at once): push chunks of encoder-rate features, get the greedy CTC ids each chunk adds; finish() gives transcribe()'s
        result for the same decoding chunk mask, frees nothing and may be repeated.  A model without the CTC head streams too: push
        returns empty lists and finish runs the attention beam.  With an AudioParser
        of norm="global" it also takes audio as it arrives: push_audio(pcm, n_samples, final) - at source_rate, converted to
        16 kHz on the GPU as it arrives (data_handler.resample.StreamResampler); None = 16 kHz, nothing is converted.
        search="prefix_beam" (needs the CTC head): a CTC prefix beam search of `beam_size` over the `frame_topk` best classes of each
        frame runs with the audio (asr_ctc_prefix_beam_chunk); push then returns the tokens by which the stable prefix grew, partial() /
        nbest() the revisable hypotheses, and finish(joint="ctc_rescore") re-ranks the n-best with the decoder.
        context (a context.ContextGraph; search="prefix_beam" only) / context_ids (the graph per utterance; None: graph 0, -1: none):
        hotword biasing of the streamed search - partial(), nbest() and finish() then report 'bias' and order by 'score'.
        lm (an lm.NgramLM; search="prefix_beam" only, not with a context): n-gram LM shallow fusion of the streamed search - partial(),
        nbest() and finish() then report 'lm_score' and order by 'score'.
        timed=True (search="greedy" only): tokens() gives every emitted character's frames, times and confidence as the audio arrives
        (confidence.TokenLog); confidence picks the measure reported as "confidence" (confidence.MEASURES).  push returns what it returns.
        beam_times=True (search="prefix_beam" only, not with a context or an LM): the search also carries every hypothesis' best single
        alignment (asr_ctc_prefix_beam_chunk_timed); nbest() entries gain "viterbi_score" and "tokens", partial() "tokens", and tokens()
        lists the best hypothesis' tokens with "final" flags.  confidence: post_max, post_min or post_mean.
        blank_skip=p in (0, 1] (search="prefix_beam" only): blank-frame skipping in front of the streamed search, with one carried bit
        per utterance - after every push bit for bit ctc_prefix_beam_search(blank_skip=p) on the frames so far (sessions.py).
        keywords (a keywords.KeywordList; any search, not with blank_skip): keyword spotting with the audio - keyword_hits() lists per
        utterance the hits so far, as spot_keywords reports them."""
        self._no_streamed_conditioning("stream")
        from ..stream import StreamingEncoder
        return StreamingEncoder(self, batch_size, parser=parser, source_rate=source_rate, search=search, beam_size=beam_size, frame_topk=frame_topk,
                                context=context, context_ids=context_ids, lm=lm, timed=timed, confidence=confidence, beam_times=beam_times,
                                blank_skip=blank_skip, keywords=keywords)

    def sessions(self, slots, parser=None, search="greedy", beam_size=5, frame_topk=10, endpoint=None, source_rate=None, context=None, lm=None,
                 timed=False, confidence="post_max", beam_times=False, blank_skip=None, keywords=None):
        """`slots` independent streaming sessions in one batch (sessions.Sessions, the owner of the streaming state and tick that
        stream() views in lock-step; needs the CTC head): each slot is opened, fed (push / push_audio), closed, finished and reopened at
        its own pace - open(b), push(feats, n_valid, final), results(b) without freeing, finish(b) - and with endpoint={...} the
        CTC endpoint rules report per slot when its speaker has stopped (endpoints()).  parser, search, beam_size, frame_topk as
        stream()'s; only 16 kHz audio.  context (search="prefix_beam" only): hotword biasing, open(b, context=i) picks the session's graph.
        lm (search="prefix_beam" only, not with a context): one n-gram LM for all slots; a reopened slot restarts on its start state.
        timed=True (search="greedy" only): tokens(b) gives slot b's characters with frames, times and confidence as the audio arrives;
        confidence picks the measure reported as "confidence".  A reopened slot starts an empty list.
        beam_times=True (search="prefix_beam" only, not with a context or an LM): as stream()'s - nbest(b) / partial(b) gain "tokens",
        tokens(b) lists slot b's best hypothesis with "final" flags; finish, drop and reopening drop the records.
        blank_skip=p (search="prefix_beam" only): as stream()'s; a reopened slot starts with a clear carry bit, and endpointing keeps
        counting every frame.
        keywords (a keywords.KeywordList; any search, not with blank_skip): one phrase list for all slots - keyword_hits(b) lists slot
        b's hits so far (final closes a match still open), a reopened slot starts an empty list."""
        self._no_streamed_conditioning("sessions")
        from ..sessions import Sessions
        return Sessions(self, slots, parser=parser, search=search, beam_size=beam_size, frame_topk=frame_topk, endpoint=endpoint, source_rate=source_rate,
                        context=context, lm=lm, timed=timed, confidence=confidence, beam_times=beam_times, blank_skip=blank_skip, keywords=keywords)

    def _no_streamed_conditioning(self, what):
        if self.interctc_condition:      # the streaming tick runs its own encoder layers, without the conditioning between them
            raise ValueError(f"model.{what}() with interctc_condition=True is not implemented: self-conditioning in the streaming encoder")

    def forward(self, input):
        """transformer_official.py:68-81 (inference-style forward; no gradients).  A batch without a transcript (only wave / wave_len)
        gets the encoder output and the CTC logits; pred / gold need tgt_for_input."""
        eng, x, wave_len, prep = self._prepare(input)
        B, T, _ = x.shape
        enc, _ = self.encode(eng, x, wave_len)
        pack = Pack()
        pack.add(encoder_out=enc.view(B, T, -1))
        if self.use_decoder and prep is not None:      # teacher forcing needs the transcript
            cross_len, Tk = self._cross(eng, input, wave_len, T)
            pred, _ = eng.decoder_fwd(prep, enc, cross_len, B, T, Tk)
            pack.add(pred=pred.view(B, -1, self.V), gold=prep[1].long())
        if self.use_ctc:
            logits = eng.ctc_lo.fwd(enc)
            pack.add(ctc_logits=logits.view(B, T, self.V))
        return pack

    def _tok_table(self, device):
        if getattr(self, "_tok_tab", None) is None or self._tok_tab[0].device != torch.device(device):
            self._tok_tab = K.token_table(self.vocab._id2token, device)
        return self._tok_tab

    def _cer_ids(self, ids, gold, hyp_len=None, ref_len=None):
        """CER in percent of a batch as a 1-element DEVICE tensor: strings, edit distance and the mean stay on
        the GPU (asr_cer) - the reference copies the ids to the host and loops over the batch every step
        (transformer_official.py:87-91, score.py:4-13)."""
        per = K.cer(ids.int().contiguous(), gold.int().contiguous(), self._tok_table(ids.device), self.vocab._token2id[self.vocab.PAD],
                    hyp_len=hyp_len, ref_len=ref_len)
        return (per.sum() * (100.0 / per.numel())).reshape(1)

    CER_BESIDE_BACKWARD = True      # False: score the step's CER on the main stream behind the optimizer (A/B, tests)

    def _cer_beside_backward(self, eng, score, keep, inline):
        """The per-step CER (five small launches, ~65 us behind the optimizer on the main stream: 1.3 % of the joint step) on the auxiliary
        stream instead, which is idle once the decoder's backward pass has joined it: it runs beside the encoder's backward pass, and iterate()
        makes the main stream wait for its event before handing the metric out.  score: closure that returns the CER tensor; keep: what it
        reads (blocks of the main stream's pool read on another stream), referenced by the model until the next step.  Returns (cer, event),
        or inline() when the step runs on one stream (or is being captured): what _cer_of takes for a score on the main stream."""
        if not (self.CER_BESIDE_BACKWARD and eng._aux_active()):
            return inline()
        if getattr(self, "_cer_event", None) is None:
            self._cer_event = torch.cuda.Event()
        # disarm: this fork is for the auxiliary stream, it must not consume a hand-over meant for the weight-gradient stream
        with E._OnAux(eng, event=self._cer_event, disarm=True):
            cer = score()
        self._cer_keep = keep
        return cer, self._cer_event

    def _cer_of(self, pg):
        """The CER tensor of what train_step returned: (cer, event) when it was computed on the auxiliary stream (the current stream then waits
        for the event), else (ids, gold) to be scored here."""
        if isinstance(pg[1], torch.cuda.Event):
            torch.cuda.current_stream().wait_event(pg[1])
            return pg[0]
        if pg[1] is None:      # already scored on the current stream
            return pg[0]
        return self._cer_ids(pg[0], pg[1])

    def _cer(self, pred, gold):
        """transformer_official.py:87-91.  Greedy ids by argmax (first index wins ties - the
        reference's topk(1) tie order at exactly-zero padded rows is implementation-defined)."""
        return self._cer_ids(pred.argmax(-1), gold)

    def cal_metrics(self, output, input):
        """transformer_official.py:83-94 on a forward() output (evaluation path)."""
        pack = Pack()
        row_nll = nll = n_valid = None
        if self.use_decoder:
            pred, gold = output.pred, output.gold
            B, To, V = pred.shape
            n_valid = (gold != PAD_ID).sum().float().reshape(1)
            row_nll, _ = K.xent_fwd_bwd(pred.reshape(B * To, V).contiguous(), gold.reshape(-1).int(), n_valid, PAD_ID, smoothing=self.label_smoothing, want_grad=False)
        if self.use_ctc:
            prep = K.dec_preprocess(input.tgt_for_input.contiguous(), SOS_ID, EOS_ID)
            nll, _ = K.ctc_fwd_bwd(output.ctc_logits.contiguous(), input.wave_len.to(torch.int32), prep[2], prep[4], self._engine.ws, want_grad=False)
        lam = self.ctc_weight
        loss = K.loss_combine(row_nll, n_valid, nll, 1.0 - lam if self.use_ctc else 1.0, lam)
        assert not torch.isinf(loss[0])
        pack.add(loss=loss[0])
        if self.use_decoder:
            pack.add(cer=self._cer(output.pred, output.gold))
        if self.use_ctc:
            # best-path CTC decoding on the device; the label strings (no sos/eos) are the reference
            cer = self._ctc_cer(output.ctc_logits.contiguous(), input.wave_len.to(torch.int32), prep[2], prep[4])
            pack.add(**({"ctc_cer": cer} if self.use_decoder else {"cer": cer}))
        return pack

    def beam_search(self, input, beam_size=5, nbest=1, decode_max_len=0, ctc_weight=0.0, joint="rescore", ctc_pre_beam=None, context=None,
                    context_ids=None, lm=None, blank_skip=None):
        """Attention-decoder beam search for a batch (Decoder.recognize_beam, transformer_official.py:
        331-434, batched on the GPU with key/value caches): per utterance a list of at most `nbest`
        {'yseq': [sos, ..., eos], 'score': float}.
        ctc_weight > 0 (joint models): the beam's hypotheses are re-ranked by ctc_weight * log p_ctc + (1 - ctc_weight) *
        log p_att (decode.joint_beam_search; entries then also carry 'att_score' and 'ctc_score').
        joint="one_pass": CTC prefix scores take part in every step of the search instead (decode.one_pass_beam_search, same result
        format; needs both heads and 0 < ctc_weight <= 1); ctc_pre_beam = attention candidates per hypothesis (default
        min(16, int(1.5 * beam_size)), at least beam_size).
        joint="ctc_rescore": the U2 two-pass search instead (decode.ctc_rescore_search; needs both heads): the CTC prefix beam search
        proposes beam_size hypotheses, one teacher-forced decoder pass re-ranks them by the same combination; 'yseq' then carries no
        sos / eos, and decode_max_len does not apply.
        context / context_ids: hotword biasing (ctc_prefix_beam_search) - joint="ctc_rescore" only, whose first pass it biases; the
        attention beam search and the other joint searches raise.
        lm (an lm.NgramLM): n-gram LM shallow fusion, under the same rule - joint="ctc_rescore" only, and not together with a context.
        blank_skip (a probability in (0, 1]): blank-frame skipping in front of the CTC prefix beam search, under the same rule."""
        from .. import decode
        if joint not in ("rescore", "one_pass", "ctc_rescore"):
            raise ValueError(f"joint must be 'rescore', 'one_pass' or 'ctc_rescore' (got {joint!r})")
        if blank_skip is not None:
            K.blank_skip_threshold(blank_skip)
            if joint != "ctc_rescore":
                what = "the attention beam search" if joint == "rescore" and not ctc_weight > 0.0 else f"joint={joint!r}"
                raise ValueError(f"blank_skip is not supported by {what}: it drops frames in front of the CTC prefix beam search - "
                                 "ctc_prefix_beam_search, beam_search(joint='ctc_rescore'), stream / sessions with search='prefix_beam'")
        if lm is not None and joint != "ctc_rescore":
            what = "the attention beam search" if joint == "rescore" and not ctc_weight > 0.0 else f"joint={joint!r}"
            raise ValueError(f"an n-gram LM (lm=...) is not supported by {what}: it is fused into the CTC prefix beam search - "
                             "ctc_prefix_beam_search, beam_search(joint='ctc_rescore'), stream / sessions with search='prefix_beam'")
        if (context is not None or context_ids is not None) and joint != "ctc_rescore":
            what = "the attention beam search" if joint == "rescore" and not ctc_weight > 0.0 else f"joint={joint!r}"
            raise ValueError(f"hotword biasing (context=...) is not supported by {what}: it biases the CTC prefix beam search - "
                             "ctc_prefix_beam_search, beam_search(joint='ctc_rescore'), stream / sessions with search='prefix_beam'")
        if joint == "one_pass":
            return decode.one_pass_beam_search(self, input, beam_size, nbest, decode_max_len, ctc_weight, ctc_pre_beam)
        if joint == "ctc_rescore":
            if ctc_pre_beam is not None:
                raise ValueError("ctc_pre_beam applies to joint='one_pass' only")
            return decode.ctc_rescore_search(self, input, beam_size, nbest, ctc_weight, context=context, context_ids=context_ids, lm=lm,
                                             blank_skip=blank_skip)
        if ctc_pre_beam is not None:
            raise ValueError("ctc_pre_beam applies to joint='one_pass' only")
        if ctc_weight > 0.0:
            return decode.joint_beam_search(self, input, beam_size, nbest, decode_max_len, ctc_weight)
        return decode.beam_search(self, input, beam_size, nbest, decode_max_len)

    def ctc_prefix_beam_search(self, input, beam_size=5, nbest=1, frame_topk=10, on_device=None, context=None, context_ids=None, lm=None,
                               beam_times=False, confidence="post_max", blank_skip=None):
        """CTC prefix beam search over the CTC head (decode.ctc_prefix_beam_search): per utterance at most `nbest`
        {'yseq': [ids], 'score': log p(yseq | x)}.  on_device: None = the device kernel when beam * (frame_topk + 1) <= 64.
        context / context_ids: hotword biasing; entries are then {'yseq', 'score', 'ctc_score', 'bias'} (decode.ctc_prefix_beam_search).
        lm: n-gram LM shallow fusion (lm.NgramLM); entries are then {'yseq', 'score', 'ctc_score', 'lm_score'}.
        beam_times=True (the device search, not with a context or an LM): entries gain 'viterbi_score' and 'tokens' - per token its frames and
        times in the hypothesis' best single alignment, the measures post_max / post_min / post_mean over them and 'confidence' (the one picked).
        blank_skip=p in (0, 1]: frames whose blank posterior and whose predecessor's are above p are dropped in front of the search."""
        from .. import decode
        return decode.ctc_prefix_beam_search(self, input, beam_size, nbest, frame_topk, on_device, context=context, context_ids=context_ids, lm=lm,
                                             beam_times=beam_times, confidence=confidence, blank_skip=blank_skip)

    def ctc_greedy_search(self, input):
        """Best-path CTC hypotheses of a batch: list of id lists (repeats merged, blanks removed)."""
        with torch.no_grad():
            out = self.forward(input)
        ids, lens = K.ctc_greedy_decode(out.ctc_logits.contiguous(), input.wave_len.to(torch.int32), PAD_ID)
        ids, lens = ids.cpu(), lens.cpu()
        return [ids[b, : int(lens[b])].tolist() for b in range(ids.shape[0])]

    def frame_seconds(self):
        """Duration of one encoder frame: lfr_n * hop / sample_rate (the low-frame-rate stacking keeps every lfr_n-th 10 ms
        feature frame; 30 ms with the AISHELL-1 defaults lfr_n = 3, sample_rate = 16000)."""
        from ..data_handler.processor import HOP
        return int(getattr(self.config, "lfr_n", 3) or 3) * HOP / float(getattr(self.config, "sample_rate", 16000) or 16000)

    def ctc_align(self, input, labels=None, confidence=None):
        """CTC forced alignment (Viterbi over the CTC head, asr_ctc_align) of a batch.
        labels=None aligns the batch's own transcripts (tgt_for_input); otherwise one list of token ids per utterance.
        Returns per utterance {"score": log-probability of the best path (-inf when the labels do not fit the frames),
        "tokens": [{"id", "token", "start_frame", "end_frame", "start_s", "end_s", "logp"}]}, where frames count encoder frames,
        start_s = start_frame * d and end_s = (end_frame + 1) * d with d = frame_seconds(), and logp is the sum of the token's
        log-probabilities over its frames.  Tokens of an utterance that cannot be aligned carry None for the frames, times and logp.
        confidence (None, True = "post_max", or one of confidence.MEASURES): every token gains "confidence" (that measure over its
        frames) and "measures" (all five), the utterance "confidence" (the mean over its tokens, None without one) - one
        asr_ctc_frame_stats and one asr_ctc_token_conf launch behind the alignment's."""
        from ..confidence import measure
        confidence = measure(confidence)
        if confidence is not None and not self.use_ctc:
            raise ValueError("confidence comes from the CTC head, and this model has none (config.ctc_weight = 0)")
        if not self.use_ctc:
            raise RuntimeError("this model has no CTC head (config.ctc_weight = 0)")
        if labels is None:
            if input.tgt_for_input is None:
                raise ValueError("ctc_align(labels=None) aligns the batch's transcripts, and this batch has none: pass labels")
            prep = K.dec_preprocess(input.tgt_for_input.contiguous(), SOS_ID, EOS_ID)
            lab, lens = prep[2].cpu(), prep[4].cpu().tolist()
            labels = [lab[b, : lens[b]].tolist() for b in range(lab.shape[0])]
        return self._align_lists(self._ctc_logits(input), input.wave_len, labels, confidence=confidence)

    def _ctc_logits(self, input):
        eng = self._ensure_engine(input.wave.device)
        was_training = eng.training
        try:
            with torch.no_grad():
                return self.forward(input).ctc_logits
        finally:
            eng.training = was_training

    def _align_lists(self, logits, wave_len, labels, alignable=None, confidence=None):
        """One asr_ctc_align launch for a batch of id lists; entries with alignable[b] False are not aligned (times None).
        confidence (a measure's name): two more launches, asr_ctc_frame_stats and asr_ctc_token_conf, over the same logits and spans."""
        B, T, V = logits.shape
        if len(labels) != B:
            raise ValueError(f"{len(labels)} label sequences for a batch of {B}")
        labels = [[int(x) for x in l] for l in labels]
        ok = [True] * B if alignable is None else list(alignable)
        for b, l in enumerate(labels):
            if ok[b] and (len(l) > 255 or any(x < 0 or x >= V for x in l)):
                raise ValueError(f"utterance {b}: labels must be at most 255 ids in [0, {V})")
        use = [l if ok[b] else [] for b, l in enumerate(labels)]
        Lmax = max([len(l) for l in use] + [0])
        lab = torch.zeros(B, Lmax, dtype=torch.int32)
        for b, l in enumerate(use):
            if l:
                lab[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
        dev = logits.device
        lab_len = torch.tensor([len(l) for l in use], dtype=torch.int32)
        in_len, lab, lab_len = wave_len.to(torch.int32).contiguous(), lab.to(dev), lab_len.to(dev)
        _, spans, tlp, score = K.ctc_align(logits, in_len, lab, lab_len, blank=PAD_ID, ws=self._engine.ws)
        conf = None
        if confidence is not None:
            from ..confidence import measures_dict, utterance
            _, _, _, lse, ent = K.ctc_frame_stats(logits, in_len, PAD_ID)
            conf = K.ctc_token_conf(logits, lab, lab_len, spans, lse, ent).cpu().tolist()
        spans, tlp, score = spans.cpu().tolist(), tlp.cpu().tolist(), score.cpu().tolist()
        d = self.frame_seconds()
        id2tok = self.vocab._id2token
        out = []
        for b, l in enumerate(labels):
            timed = ok[b] and score[b] != float("-inf")
            toks = []
            for i, x in enumerate(l):
                st, en = (spans[b][i][0], spans[b][i][1]) if timed else (None, None)
                toks.append({"id": x, "token": id2tok[x] if 0 <= x < len(id2tok) else None, "start_frame": st, "end_frame": en,
                             "start_s": st * d if timed else None, "end_s": (en + 1) * d if timed else None,
                             "logp": tlp[b][i] if timed else None})
                if conf is not None:
                    m = measures_dict(conf[b][i]) if timed else None
                    toks[-1]["measures"], toks[-1]["confidence"] = m, (m[confidence] if m else None)
            out.append({"score": score[b] if ok[b] else None, "tokens": toks})
            if conf is not None:
                out[-1]["confidence"] = utterance(t["confidence"] for t in toks)
        return out

    def transcribe(self, input, beam_size=5, ctc_weight=None, timestamps=True, joint="rescore", context=None, context_ids=None, lm=None, confidence=None,
                   blank_skip=None):
        """Audio in, text out, for a batch that needs only wave / wave_len.  The search follows the model's heads: joint model =
        beam_search(ctc_weight = config.ctc_weight unless given), CTC-only model = ctc_prefix_beam_search, attention-only model =
        beam_search (no timestamps: they come from the CTC head).  Returns per utterance {"text", "ids", "score", "tokens"}: ids of
        the best hypothesis without sos / eos, text = their vocabulary tokens joined (pad / sos / eos dropped), score = the search's
        score, tokens = ctc_align's token list of the hypothesis (one launch for the batch; None when timestamps=False).  A hypothesis
        the CTC head cannot spell (infeasible for the frames, containing the blank id, longer than 255) keeps its text with None times.
        joint: the joint model's search, "rescore" (two-pass), "one_pass" or "ctc_rescore" (CTC n-best re-ranked by the decoder)
        (beam_search(joint=...)); "one_pass" and "ctc_rescore" need both heads.
        context / context_ids: hotword biasing of the CTC prefix beam search (a CTC-only model, or joint="ctc_rescore"; any other
        search raises ValueError); the result dicts gain "bias".
        lm: n-gram LM shallow fusion in the CTC prefix beam search, under the same rule; the result dicts gain "lm_score".
        blank_skip (a probability in (0, 1]): blank-frame skipping in front of the CTC prefix beam search, under the same rule; "score"
        then sums over the kept frames, and the token times still come from ctc_align over all frames.
        confidence (None, True = "post_max", or one of confidence.MEASURES; needs timestamps and the CTC head, ValueError otherwise):
        every token gains "confidence" and "measures", the result "confidence" (ctc_align's); tokens without times carry None."""
        from ..confidence import measure
        confidence = measure(confidence)
        if confidence is not None and not timestamps:
            raise ValueError("confidence needs timestamps=True: a token's confidence is taken over the frames of its alignment")
        if confidence is not None and not self.use_ctc:
            raise ValueError("confidence comes from the CTC head, and this model has none (config.ctc_weight = 0)")
        if joint not in ("rescore", "one_pass", "ctc_rescore"):
            raise ValueError(f"joint must be 'rescore', 'one_pass' or 'ctc_rescore' (got {joint!r})")
        if joint in ("one_pass", "ctc_rescore") and not (self.use_decoder and self.use_ctc):
            raise RuntimeError(f"joint={joint!r} needs a model with both the attention decoder and the CTC head")
        if timestamps and not self.use_ctc:
            raise ValueError("timestamps come from the CTC head, and this model has none (config.ctc_weight = 0)")
        if self.use_decoder:
            w = float(getattr(self.config, "ctc_weight", 0.0)) if ctc_weight is None else float(ctc_weight)
            hyps = self.beam_search(input, beam_size, 1, ctc_weight=w if self.use_ctc else 0.0, joint=joint, context=context, context_ids=context_ids, lm=lm,
                                    blank_skip=blank_skip)
        else:
            hyps = self.ctc_prefix_beam_search(input, beam_size, 1, context=context, context_ids=context_ids, lm=lm, blank_skip=blank_skip)
        ids, scores, biases = [], [], []
        bias_key = "lm_score" if lm is not None else "bias"
        for h in hyps:
            biases.append(float(h[0][bias_key]) if h and bias_key in h[0] else 0.0)
            if not h:
                ids.append([])
                scores.append(float("-inf"))
                continue
            seq = list(h[0]["yseq"])
            if self.use_decoder and joint != "ctc_rescore":      # the CTC n-best is spelled without sos / eos
                seq = seq[1:] if seq and seq[0] == SOS_ID else seq
                seq = seq[:-1] if seq and seq[-1] == EOS_ID else seq
            ids.append(seq)
            scores.append(float(h[0]["score"]))
        return self._hyp_dicts(ids, scores, timestamps, lambda: self._ctc_logits(input), input.wave_len,
                               biases if context is not None or lm is not None else None, bias_key, confidence=confidence)

    def transcribe_long(self, parser, wav, wav_len, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
                        max_segment_s=20.0, **transcribe_kw):
        """Whole recordings in, text out (longform.transcribe_long): wav (B, S) f32 samples (at source_rate when given, else 16 kHz) are
        cut at their pauses by the energy VAD (vad.EnergyVad; None: Kaldi's defaults), the segments of each recording go through
        transcribe(**transcribe_kw) in time order, batch_size at a time, and come back on the recording's time axis: per recording
        {"text", "ids", "duration_s", "segments": [{"start_s", "end_s", "start_sample", and transcribe's result for the segment}]}."""
        from ..longform import transcribe_long
        return transcribe_long(self, parser, wav, wav_len, vad=vad, batch_size=batch_size, source_rate=source_rate, min_silence_s=min_silence_s,
                               min_speech_s=min_speech_s, pad_s=pad_s, max_segment_s=max_segment_s, **transcribe_kw)

    def align_long(self, parser, wav, wav_len, texts, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
                   max_segment_s=20.0, confidence="post_mean", max_bytes=4 << 30, filler=None, filler_scope="lines"):
        """Whole recordings and their transcripts in, per-token and per-line times out (align_long.align_long): the VAD's segments go
        through the CTC head in time order, their frames are laid end to end on the device, and one asr_ctc_align_long launch aligns every
        recording's transcript (a string, a list of lines or a list of id lists; up to 8192 tokens) to them.  Per recording {"score",
        "duration_s", "frames", "tokens", "lines", "segments"}; a transcript that does not fit its frames comes back with None times.
        filler (a penalty in nats; None = off) lets frames the transcript does not cover rest in wide blanks in front of every line
        (filler_scope "lines") or token ("tokens") and behind the last token (asr_ctc_align_long_filler): the results gain "fillers" and
        "filler_frames"."""
        from ..align_long import align_long
        return align_long(self, parser, wav, wav_len, texts, vad=vad, batch_size=batch_size, source_rate=source_rate, min_silence_s=min_silence_s,
                          min_speech_s=min_speech_s, pad_s=pad_s, max_segment_s=max_segment_s, confidence=confidence, max_bytes=max_bytes, filler=filler,
                          filler_scope=filler_scope)

    def spot_keywords(self, input, keywords):
        """Keyword spotting on the CTC posteriors (keywords.spot_keywords; needs the CTC head, ValueError before any launch otherwise):
        every phrase of `keywords` (a keywords.KeywordList) against every frame of the batch, with a free start and a free end - the
        encoder and the CTC projection as ctc_align runs them, then asr_ctc_frame_stats, asr_kws_search and asr_kws_compact.
        Returns per utterance {"hits": [{"keyword", "phrase", "ids", "start_frame", "end_frame", "start_s", "end_s", "score",
        "confidence"}], "dropped"}: score = the log-probability of the phrase's best alignment ending on end_frame, confidence =
        exp(score / L), start_frame = the last frame of the first character's run, times as ctc_align's; the hits sorted by
        (end_frame, keyword); dropped = the hits past hits_per_keyword or the list's max_hits."""
        from ..keywords import spot_keywords
        return spot_keywords(self, input, keywords)

    def spot_long(self, parser, wav, wav_len, keywords, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
                  max_segment_s=20.0):
        """Keyword spotting over whole recordings (keywords.spot_long): transcribe_long's segments and batches with spot_keywords in
        place of transcribe.  Per recording {"hits", "dropped", "duration_s", "segments"}: hit times on the recording's clock, frames
        relative to the hit's "segment"; a recording without speech has hits []."""
        from ..keywords import spot_long
        return spot_long(self, parser, wav, wav_len, keywords, vad=vad, batch_size=batch_size, source_rate=source_rate, min_silence_s=min_silence_s,
                         min_speech_s=min_speech_s, pad_s=pad_s, max_segment_s=max_segment_s)

    def consensus(self, input, search="ctc_prefix_beam", beam_size=5, nbest=5, posterior_scale=1.0, alts=4, **search_kwargs):
        """Consensus decoding of a batch's n-best lists (consensus.model_consensus): the lists of ctc_prefix_beam_search ("ctc_prefix_beam";
        context=, lm=, blank_skip= pass through) or beam_search ("attention_beam"; sos / eos stripped) are weighted by
        consensus.nbest_weights(their scores, posterior_scale) and voted on the device (asr_nbest_consensus).  Returns per utterance
        {"text", "ids" (the consensus string), "mbr_ids" (the minimum-Bayes-risk entry), "mbr_rank", "best_ids" (rank 0), "confidence" (per
        token of mbr_ids: the posterior mass of the entries that agree with it), "slots" (the confusion network: consensus.consensus_ids),
        "nbest" (what the search returned)}.  ValueError before any launch for nbest above 64 or a posterior_scale that is not finite
        and > 0; a hypothesis above 256 tokens raises before the votes."""
        from ..consensus import model_consensus
        return model_consensus(self, input, search=search, beam_size=beam_size, nbest=nbest, posterior_scale=posterior_scale, alts=alts, **search_kwargs)

    def rescore(self, input, weights, search="attention_beam", beam_size=5, nbest=5, lm=None, **search_kwargs):
        """The n-best lists of a batch re-ranked by a weighted sum of scores (rescore.rescore): weights = {column: w} over the scores the
        search reports ("ctc_score", "att_score", "bias", "lm_score", "score"), "lm" (the n-gram LM score of the finished string, all entries
        in one launch of asr_lm_score_nbest; lm= an NgramLM compiled with weight=1.0, ins=0.0) and "len" (the token count).  Returns the
        lists re-ordered, every entry a copy with "score" = its total (-inf: unscorable), "first_rank" and "lm" / "len" where used."""
        from ..rescore import model_rescore
        return model_rescore(self, input, weights, search=search, beam_size=beam_size, nbest=nbest, lm=lm, **search_kwargs)

    def tune(self, batches, grid, search="attention_beam", beam_size=10, nbest=10, lm=None, **search_kwargs):
        """The error counts of every point of a rescore.Grid of weight vectors over a dev set: every pack goes through the search once, its
        entries through asr_edit_align (counts only) and asr_nbest_sweep.  Returns a rescore.SweepResult (cer, ser, best, best_weights,
        rank0_cer, oracle_cer, save)."""
        from ..rescore import model_tune
        return model_tune(self, batches, grid, search=search, beam_size=beam_size, nbest=nbest, lm=lm, **search_kwargs)

    def evaluate(self, batches, search="transcribe", nbest=1, scorer=None, consensus=False, posterior_scale=1.0, rescore=None, rescore_lm=None, **search_kwargs):
        """Token-level scoring of a test set (scoring.evaluate): every pack of `batches` (what the loader yields) goes through `search` -
        "transcribe" (1-best; transcribe(pack, timestamps=False, **search_kwargs), so joint=, context=, lm=, blank_skip= pass through),
        "ctc_prefix_beam" (ctc_prefix_beam_search(pack, beam_size, nbest, ...)) or "attention_beam" (beam_search(pack, beam_size, nbest,
        ...)) - and its hypotheses are aligned on the device (asr_edit_align) against the gold ids cal_metrics scores against.  Returns the
        scoring.Scorer (a new one, or `scorer` with the batches added): summary() has the corpus CER with its substitutions, deletions and
        insertions, the sentence error rate and, with nbest > 1, the oracle CER of the lists.  consensus=True (the two n-best searches):
        also mbr_cer, consensus_cer and mbr_rank_hist, from consensus.consensus_ids over the lists with their scores and posterior_scale.
        rescore={column: w} (the two n-best searches; rescore_lm= the NgramLM of a column "lm"): the lists are re-ranked by self.rescore's
        rule first, so the scores are those of the rescored rank 0 and a consensus sees the new totals."""
        from ..scoring import evaluate
        return evaluate(self, batches, search=search, nbest=nbest, scorer=scorer, consensus=consensus, posterior_scale=posterior_scale, rescore=rescore,
                        rescore_lm=rescore_lm, **search_kwargs)

    def _hyp_dicts(self, ids, scores, timestamps, ctc_logits, wave_len, biases=None, bias_key="bias", confidence=None):
        """transcribe's result dicts for the best ids / score of each utterance; ctc_logits() -> (B, T, V) is called for timestamps only.
        biases (hotword-biased searches, or searches with an n-gram LM): the "bias" (bias_key="lm_score": the "lm_score") of each result."""
        id2tok = self.vocab._id2token
        out = [{"text": "".join(id2tok[x] for x in seq if x not in (PAD_ID, SOS_ID, EOS_ID)), "ids": seq, "score": sc, "tokens": None}
               for seq, sc in zip(ids, scores)]
        if biases is not None:
            for o, bias in zip(out, biases):
                o[bias_key] = bias
        if timestamps:
            V = self.V
            ok = [len(seq) <= 255 and all(0 <= x < V and x != PAD_ID for x in seq) for seq in ids]
            al = self._align_lists(ctc_logits(), wave_len, ids, alignable=ok, confidence=confidence)
            for o, a in zip(out, al):
                o["tokens"] = a["tokens"]
                if confidence is not None:
                    o["confidence"] = a["confidence"]
        return out

    def _ctc_cer(self, logits, wave_len, labels32, lab_len):
        ids, lens = K.ctc_greedy_decode(logits, wave_len, PAD_ID)
        return self._cer_ids(ids, labels32, hyp_len=lens, ref_len=lab_len)

    def train_step(self, input, loss_scale=1.0, count_hook=None):
        """Forward + backward into the flat gradient buffer (no optimizer).  Returns the metrics
        tensor [loss, ce, ctc] (device) and, for CER, (pred, gold) or None.
        count_hook (data parallelism, dist.DataParallel): called as count_hook(n_valid, B) right after the label
        preprocessing; it starts the all-reduce of [non-pad token count, batch size] and returns an object whose wait()
        yields the two GLOBAL values as 1-element device tensors - the loss kernels then normalise by those."""
        if self.cr_ctc_weight > 0.0 and int(input.wave.shape[0]) % 2:      # before anything is launched
            raise ValueError(f"cr_ctc_weight > 0 takes the two views of every utterance, rows p and p + B/2: a batch of {int(input.wave.shape[0])} rows is odd")
        eng, x, wave_len, prep = self._prepare(input, training=self.training)
        B, T, _ = x.shape
        lam = self.ctc_weight
        ys_in, ys_out, labels32, dec_len, lab_len, n_valid = prep
        pending = count_hook(n_valid, B) if count_hook is not None else None
        zero, self._zero_lazy = (self._flat.g if getattr(self, "_zero_lazy", False) else None), False
        eng.refresh_transposes(zero=zero)      # W^T copies for this step's input-gradient GEMMs (side stream, beside the forward pass)
        batch_div = None
        inter = None
        w_inter = self.interctc_weight if (self.interctc_layers and self.use_ctc and not self.use_decoder) else 0.0
        if w_inter > 0.0:
            # the listed layers' CTC terms are scaled on the way up, so the global batch size is needed in front of the encoder here
            if pending is not None:
                n_valid, batch_div = pending.wait()
                pending = None
            share = w_inter / len(self.interctc_layers) * loss_scale
            inter = dict(labels32=labels32, lab_len=lab_len, grad_scale=share if batch_div is not None else share / float(B), grad_scale_div=batch_div)
        enc, ecache = self.encode(eng, x, wave_len, training=True, interctc=inter)
        if pending is not None:
            n_valid, batch_div = pending.wait()
        row_nll = nll = None
        d_enc = None
        pg = None
        ctc_done = None
        lam_g = lam * (1.0 - w_inter)      # intermediate CTC: the final head carries 1 - w of the CTC term
        ctc_scale = dict(grad_scale=lam_g * loss_scale, grad_scale_div=batch_div) if batch_div is not None else dict(grad_scale=lam_g * loss_scale / float(B))
        ctc_async = (self.use_decoder and self.use_ctc and eng._aux_active() and not eng.deterministic)
        if self.use_decoder:
            cross_len, Tk = self._cross(eng, input, wave_len, T)
        if ctc_async:      # joint model: the CTC branch runs beside the decoder's forward pass
            eng.decoder_kv_async(prep, enc, B, T, Tk)      # ... behind the K|V projections the decoder's first cross-attention waits for
            nll, d_enc, ctc_done = eng.ctc_branch_async(enc, wave_len, labels32, lab_len, B, T, **ctc_scale)
        if self.use_decoder:
            pred, dcache = eng.decoder_fwd(prep, enc, cross_len, B, T, Tk)
            # the greedy ids of the step's CER come out of the loss kernel (it reads every row anyway; the gradient overwrites the logits in place)
            ids = torch.empty(ys_out.shape, dtype=torch.int32, device=pred.device) if self.cer_in_iterate else None
            w_ce = (1.0 - lam) if self.use_ctc else 1.0
            row_nll, dpred = K.xent_fwd_bwd(pred, ys_out.reshape(-1), n_valid, PAD_ID, smoothing=self.label_smoothing, grad_scale=w_ce * loss_scale, dlogits=pred,
                                            argmax=ids)
            if ids is not None:
                pg = (ids, ys_out)
        if self.use_ctc and not ctc_async:
            # CTC-only model: the step's CER (the reference's trainer reads metrics.cer every step, Trainer/trainer11.py:73-75) is scored on the
            # greedy CTC path, which the loss kernels hand out (the gradient overwrites the logits in place)
            path = torch.empty(B, T, dtype=torch.int32, device=enc.device) if (self.cer_in_iterate and not self.use_decoder) else None
            mwer = {}
            if self.mwer_weight > 0.0:      # scaled as the CTC term is: by the batch, or by the global batch on the device
                mwer = dict(mwer_grad_scale=self.mwer_weight * loss_scale / (1.0 if batch_div is not None else float(B)))
            cr = {}
            if self.cr_ctc_weight > 0.0:      # a mean over the pairs: cr_ctc_weight * loss_scale / (B / 2), or over the global pairs on the device
                cr = dict(cr_grad_scale=2.0 * self.cr_ctc_weight * loss_scale / (1.0 if batch_div is not None else float(B)))
            nll, d_enc = eng.ctc_fwd_bwd(enc, wave_len, labels32, lab_len, B, T, best_path=path, **ctc_scale, **mwer, **cr)
            if path is not None:      # collapse the greedy path and score it against the label strings, as cal_metrics does for a CTC-only model
                def score():
                    ids, lens = K.ctc_collapse(path, wave_len, PAD_ID)
                    return self._cer_ids(ids, labels32, hyp_len=lens, ref_len=lab_len)
                pg = self._cer_beside_backward(eng, score, (path, wave_len, labels32, lab_len), inline=lambda: (score(), None))
        if self.use_decoder:
            if d_enc is None:
                d_enc = torch.zeros_like(enc)
            eng.decoder_bwd(dcache, dpred, d_enc, d_enc_ready=ctc_done)
            if pg is not None:
                pg = self._cer_beside_backward(eng, lambda: self._cer_ids(ids, ys_out), pg, inline=lambda: pg)      # inline: (ids, gold), scored by _cer_of
        eng.encoder_bwd(ecache, d_enc)
        loss = K.loss_combine(row_nll, n_valid, nll, (1.0 - lam) if self.use_ctc else 1.0, lam)
        self._mwer_mean = None
        if self.mwer_weight > 0.0 and self.use_ctc and not ctc_async:
            # the MWER term beside the combined loss: mwer_weight * the mean risk of the batch (no device-to-host copy, no sync)
            risk = eng.last_mwer[4]
            self._mwer_mean = risk.sum() / (batch_div[0] if batch_div is not None else float(B))
            loss = loss.clone()
            loss[0] += self.mwer_weight * self._mwer_mean
        self._cr_mean = None
        if self.cr_ctc_weight > 0.0 and self.use_ctc and not ctc_async:
            # the consistency term beside the combined loss: cr_ctc_weight * the mean over the pairs (no device-to-host copy, no sync);
            # metrics.cr is the mean over THIS batch's pairs, the loss under data parallelism this rank's share of the global mean
            cr_sum = eng.last_cr[1].sum()
            self._cr_mean = cr_sum / float(B // 2)
            loss = loss.clone()
            loss[0] += self.cr_ctc_weight * (2.0 * cr_sum / batch_div[0] if batch_div is not None else self._cr_mean)
        self._interctc_mean = None
        if w_inter > 0.0:
            # (1 - w) CTC + w * the mean of the listed layers' CTC losses, combined on the device (no device-to-host copy, no sync); both
            # terms are means over THIS batch, as the CTC term of loss_combine is
            self._interctc_mean = eng.last_interctc.sum() / float(len(self.interctc_layers) * B)
            loss = loss.clone()
            loss[0] = (1.0 - w_inter) * loss[0] + w_inter * self._interctc_mean
        return loss, pg

    def interctc_losses(self, input):
        """The CTC loss of every utterance at the listed layers and at the top, in evaluation mode (no dropout) and without a gradient:
        {"layers": the config's interctc_layers, "interctc": one list of B losses per listed layer, "ctc": the B final losses}.  With
        interctc_condition the conditioning runs, as in every inference path.  The definition is tests/interctc_ref.py."""
        if self.use_decoder or not self.use_ctc or not self.interctc_layers:
            raise ValueError("interctc_losses needs the CTC-only model (TransformerCTC) with interctc_layers")
        eng, x, wave_len, prep = self._prepare(input, training=False)
        B, T, _ = x.shape
        labels32, lab_len = prep[2], prep[4]
        with torch.no_grad():
            enc, cache = self.encode(eng, x, wave_len, interctc=dict(labels32=labels32, lab_len=lab_len, grad_scale=0.0, grad_scale_div=None,
                                                                    want_grad=False))
            nll, _ = eng.ctc_fwd_bwd(enc, wave_len, labels32, lab_len, B, T, 0.0, want_grad=False)
        return {"layers": self.interctc_layers, "interctc": eng.last_interctc.cpu().tolist(), "ctc": nll.cpu().tolist()}

    def mwer_risk(self, input, nbest=None, beam_size=None, frame_topk=None, blank_skip=None):
        """The figures MWER training lowers, without a gradient: per utterance {"risk": the expected number of errors over the n-best list
        of the device prefix beam search, "errors": the entries' distances to the transcript, "posteriors": their share of the list's
        probability (0 for an entry that does not take part), "nbest": the id lists}.  The defaults are the config's mwer_* keys.
        Evaluation mode (no dropout); the definition is tests/mwer_ref.py on ctc_prefix_beam_search's lists."""
        d = self._mwer
        _, m = mwer_settings(0.0, d["nbest"] if nbest is None else nbest, d["beam"] if beam_size is None else beam_size,
                             d["frame_topk"] if frame_topk is None else frame_topk, blank_skip)
        if blank_skip is None:
            m["thr"] = d["thr"]
        if self.use_decoder or not self.use_ctc:
            raise ValueError("mwer_risk needs the CTC-only model (TransformerCTC)")
        eng = self._ensure_engine(input.wave.device)
        was_training, eng.training = eng.training, False
        try:
            with torch.no_grad():
                out = self.forward(input)
        finally:
            eng.training = was_training
        logits = out.ctc_logits.contiguous()
        B, T, V = logits.shape
        wave_len = input.wave_len.to(torch.int32).contiguous()
        prep = K.dec_preprocess(input.tgt_for_input.contiguous(), SOS_ID, EOS_ID)
        labels32, lab_len = prep[2], prep[4]
        vals, ids, blank_lp = K.ctc_frame_topk(logits.view(B * T, V), min(m["frame_topk"], V), PAD_ID)
        search_len = wave_len
        if m["thr"] is not None:
            vals, ids, blank_lp, search_len, _ = K.ctc_blank_skip_compact(vals, ids, blank_lp, wave_len, m["thr"], B, T)
        Lh = min(T, K.MWER_MAX_LEN, 2 * labels32.shape[1] + 8)
        tok, ln, _ = K.ctc_prefix_beam(vals, ids, blank_lp, search_len, B, T, m["beam"], m["nbest"], PAD_ID, max_len=Lh)
        res = K.ctc_mwer(logits, wave_len, tok, ln, labels32, lab_len, blank=PAD_ID, want_grad=False)
        tok, ln, err, post, risk = (t.cpu().tolist() for t in (tok, ln, res["err"], res["post"], res["risk"]))
        return [{"risk": risk[b], "errors": [err[b][r] for r in range(m["nbest"]) if ln[b][r] >= 0],
                 "posteriors": [post[b][r] for r in range(m["nbest"]) if ln[b][r] >= 0],
                 "nbest": [tok[b][r][:min(ln[b][r], Lh)] for r in range(m["nbest"]) if ln[b][r] >= 0]} for b in range(B)]

    def iterate(self, input, optimizer=None, is_train=True):
        """transformer_official.py:96-104: forward, metrics, and - when training - zero_grad,
        backward, clip_grad_norm_(5.0), optimizer.step()."""
        if optimizer is None or not is_train:
            with torch.no_grad():
                output = self.forward(input)
                return self.cal_metrics(output, input), None
        if self._ema_active:
            raise RuntimeError("iterate(is_train=True) inside ema_weights(): the parameters are swapped with their average")
        self._ensure_engine(input.wave.device)
        optimizer.zero_grad()
        if getattr(optimizer, "fused_step", None) is None or not getattr(optimizer, "keeps_grad_views", False):
            # a stock torch.optim optimizer (or the reference's own NoamOpt) sets every .grad to None in zero_grad():
            # re-attach the views of the flat gradient buffer, or clip / step would see no gradients at all
            self._grads_checked = False
        self.zero_flat_grads()
        loss, pg = self.train_step(input)
        fused = getattr(optimizer, "fused_step", None)
        if fused is not None:
            fused(self._flat, CLIP_NORM)                      # sumsq + clip + Noam + Adam, 3 launches
        else:                                                 # any torch.optim-style optimizer
            torch.nn.utils.clip_grad_norm_(self.parameters(), CLIP_NORM)
            optimizer.step()
            self._flat.refresh_lowp()
            if self._flat.ema is not None:
                self._ema_after_step(optimizer)
        metrics = Pack()
        metrics.add(loss=loss[0])
        if self.use_decoder and self.use_ctc:
            metrics.add(ce=loss[1], ctc=loss[2])
        if pg is not None:
            metrics.add(cer=self._cer_of(pg))                 # no device-to-host copy, no sync
        if getattr(self, "_mwer_mean", None) is not None:
            metrics.add(mwer=self._mwer_mean)                 # the mean risk of the batch, in errors per utterance
        if getattr(self, "_cr_mean", None) is not None:
            metrics.add(cr=self._cr_mean)                     # the mean consistency term of the batch's pairs
        if getattr(self, "_interctc_mean", None) is not None:
            metrics.add(interctc=self._interctc_mean)         # the mean CTC loss of the listed middle layers
        return metrics, None

    def greedy_search(self, input, decode_max_len=0):
        """transformer_official.py:106-107 is an empty stub in the reference; here: beam search with one beam."""
        return self.beam_search(input, 1, 1, decode_max_len)

    @classmethod
    def get_default_config(cls):
        class ModelConfig(BaseConfig):      # transformer_official.py:115-122 (+ the additions above)
            d_model = 512
            hidden_size = 64
            ff_size = 1024
            num_head = 8
            dropout = 0.1
            layer_num = 6
            share_weight = False
            ctc_weight = 0.0
            label_smoothing = 0.0
            cross_mask = "ref_compat"
            dtype = "bf16"
            attn_window = -1
            chunk_size = 0                  # encoder chunk mask in training: 0 = full, > 0 = static chunk, -1 = dynamic (encoder_mask)
            left_chunks = -1                # chunks of left context, -1 = all
            decoding_chunk_size = None      # inference mask: None = chunk_size when static, else full; 0 = full
            decoding_left_chunks = None     # None = left_chunks when the chunk is static, else -1
            ema_decay = 0.0                 # > 0: keep an exponential moving average of the parameters with this decay (0 = off, nothing allocated)
            ema_warmup = True               # the decay of step s is min(ema_decay, (1 + s) / (10 + s))
            mwer_weight = 0.0               # > 0 (TransformerCTC): the loss gains mwer_weight * mean expected errors over the model's own n-best list
            mwer_nbest = 4                  # entries of the list, in [2, mwer_beam]
            mwer_beam = 4                   # beam of the device prefix beam search that makes the list
            mwer_frame_topk = 7             # classes per frame the search looks at: mwer_beam * (mwer_frame_topk + 1) <= 64
            mwer_blank_skip = None          # a probability in (0, 1]: blank-frame skipping in front of that search
            cr_ctc_weight = 0.0             # > 0 (TransformerCTC): batches hold two views per utterance; the loss gains cr_ctc_weight * mean consistency term
            interctc_weight = 0.0           # w in (0, 1) (TransformerCTC): the loss becomes (1 - w) CTC + w * the mean CTC loss of interctc_layers
            interctc_layers = ()            # 1-based encoder layers in [1, layer_num - 1], strictly increasing; "3" / "2,4" from the command line
            interctc_condition = False      # self-conditioning at those layers: adds encoder.conditioning_layer.weight (d_model, V)

        return ModelConfig


class TransformerOffical(_SpeechTransformer):
    """Encoder-decoder with CE (and CTC when config.ctc_weight > 0)."""
    USE_DECODER = True


class TransformerCTC(_SpeechTransformer):
    """Encoder + CTC head only (BASELINE.json config 2)."""
    USE_DECODER = False
