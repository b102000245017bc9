"""Intermediate CTC with self-conditioning: the definition (torch on the CPU, float64 unless told otherwise).

The config keys interctc_weight = w, interctc_layers and interctc_condition of TransformerCTC.  With h_l the output of encoder layer l
(1-based, post-LN, padded rows exactly zero: oracle/ref_model.py:encoder_forward), for every listed layer l

    z_l = ctc_lo(h_l)                                   the SHARED head
    L_l = R.ctc_loss(z_l, wave_len, labels, lab_len)    the sum over the utterances / B, as the final loss
    if interctc_condition:
        p_l = softmax(z_l) on the frames t < wave_len[b], exactly 0 on the others
        h_l <- h_l + p_l Wc^T                           Wc = encoder.conditioning_layer.weight (d_model, V), one matrix, NO bias
    loss = (1 - w) L_final + w mean_l L_l

No bias (a bias would put a non-zero vector on the padded rows), no dropout on the conditioning; the conditioning is part of the model and
runs in inference, the intermediate losses are training only.  encoder() below is R.encoder_forward with that hook after
`feed_forward(...) * non_pad`, built from R's own pieces.  This is the project's own definition: parity with ESPnet, WeNet or icefall
(none of them at hand) is not pinned.

softmax_rows / softmax_bwd_add state what the two kernels of csrc/interctc.hip compute on (B, T, V) frames."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R

COND = "encoder.conditioning_layer.weight"


# ------------------------------------------------------------------------------------------------ the kernels
def softmax_rows(z, in_len):
    """z (B, T, V), in_len (B): softmax over V on the frames t < in_len[b] (clamped to [0, T]), zeros on the others.  A -inf entry
    gives 0; a row whose maximum is not finite gives zeros."""
    B, T, V = z.shape
    keep = torch.arange(T).unsqueeze(0) < torch.as_tensor(np.clip(np.asarray(in_len), 0, T)).view(-1, 1)
    keep = keep & torch.isfinite(z.max(dim=-1).values)
    p = torch.softmax(torch.where(keep.unsqueeze(-1), z, torch.zeros_like(z)), dim=-1)
    return p * keep.unsqueeze(-1).to(z.dtype)


def softmax_bwd(p, dp, in_len):
    """The closed form of the softmax backward on the frames t < in_len[b], zeros on the others: p (dp - sum_u p[u] dp[u])."""
    B, T, V = p.shape
    keep = (torch.arange(T).unsqueeze(0) < torch.as_tensor(np.clip(np.asarray(in_len), 0, T)).view(-1, 1)).unsqueeze(-1).to(p.dtype)
    return p * (dp - (p * dp).sum(dim=-1, keepdim=True)) * keep


def make_case(B, T, V, spread, lens=None, seed=0):
    """(logits, dp, prior gradient) float32 numpy (B, T, V) and in_len (B) int32: logits spread * N(0, 1), dp and the prior N(0, 1)."""
    g = np.random.default_rng(1000 * seed + 97 * B + 13 * T + V)
    z = (spread * g.standard_normal((B, T, V))).astype(np.float32)
    dp = g.standard_normal((B, T, V)).astype(np.float32)
    prior = g.standard_normal((B, T, V)).astype(np.float32)
    in_len = np.full(B, T, np.int32) if lens is None else np.asarray(lens, np.int32)
    return z, dp, prior, in_len


# ------------------------------------------------------------------------------------------------ the model
def encoder(sd, cfg, wave, wave_len, layers=(), condition=False, round_p=None):
    """R.encoder_forward with the hook.  Returns (encoder output, {l: z_l}).  round_p: a dtype the posteriors are rounded to before
    the conditioning product (the bf16 engine stores them in bf16); None: not rounded."""
    B, T, _ = wave.shape
    keep = R.valid_mask(wave_len, T)
    non_pad = keep.unsqueeze(-1).to(wave.dtype)
    masked = (~keep).unsqueeze(1).expand(B, T, T)
    d = cfg.d_model
    x = F.linear(wave, sd["encoder.linear_in.weight"], sd["encoder.linear_in.bias"])
    x = F.layer_norm(x, (d,), sd["encoder.layer_norm_in.weight"], sd["encoder.layer_norm_in.bias"], R.LN_EPS)
    x = x + R.positional_encoding(T, d, wave.dtype).unsqueeze(0)
    inter = {}
    for i in range(cfg.layer_num):
        pre = f"encoder.layer_stack.{i}."
        x = R.multi_head_attention(sd, pre + "slf_attn.", x, x, masked, cfg.num_head, cfg.hidden_size) * non_pad
        x = R.feed_forward(sd, pre + "pos_ffn.", x) * non_pad
        if (i + 1) in layers:
            z = R.ctc_logits(sd, x)
            inter[i + 1] = z
            if condition:
                p = torch.softmax(z, dim=-1) * non_pad
                if round_p is not None:      # a straight-through rounding: the value the engine stores, the gradient of the unrounded one
                    p = p + (p.detach().to(round_p).to(p.dtype) - p.detach())
                x = x + F.linear(p, sd[COND])
    return x, inter


def losses(sd, cfg, batch, w, layers, condition, round_p=None):
    """dict(loss, ctc: L_final, inter: [L_l], enc_out, per_utt: (n_layers + 1, B) the per-utterance losses, the final one last)."""
    enc, inter = encoder(sd, cfg, batch["wave"], batch["wave_len"], layers, condition, round_p)
    logits = R.ctc_logits(sd, enc)
    args = (batch["wave_len"], batch["tgt_for_input"], batch["tgt_len"])
    ctc = R.ctc_loss(logits, *args)
    li = [R.ctc_loss(inter[l], *args) for l in layers]
    loss = ctc if not layers else (1.0 - w) * ctc + w * torch.stack(li).mean()

    def per_utt(z):
        logp = F.log_softmax(z, dim=-1).transpose(0, 1)
        return F.ctc_loss(logp, batch["tgt_for_input"], batch["wave_len"], batch["tgt_len"], blank=R.PAD_ID, reduction="none")
    return dict(loss=loss, ctc=ctc, inter=li, enc_out=enc, per_utt=torch.stack([per_utt(inter[l]) for l in layers] + [per_utt(logits)]))


def init_cond(d_model, V, seed=0, dtype=torch.float32):
    """Xavier-uniform Wc (d_model, V)."""
    g = torch.Generator().manual_seed(seed)
    bound = (6.0 / (d_model + V)) ** 0.5
    return (torch.rand(d_model, V, generator=g, dtype=dtype) * 2 - 1) * bound
