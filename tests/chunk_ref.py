"""Host restatement of the chunk-masked encoder (asr_hip.h: asr_sdpa_chunk_fwd) for the chunk tests.

The mask is written once, densely, from its definition; the encoder and the losses are oracle.ref_model's pieces
(multi_head_attention, feed_forward, positional_encoding, ce_loss, ctc_loss) with that mask; gradients come from torch autograd
on the CPU (fp32 / fp64).  Nothing here runs on the GPU.
"""
import torch
import torch.nn.functional as F

from oracle import ref_model as R


def chunk_visible(Tq, Tk, chunk, left_chunks, k_len=None):
    """(Tq, Tk) bool, or (B, Tq, Tk) with k_len: True where query i sees key j:
    j < k_len[b]  and  j < (i // C + 1) * C  and  (left < 0  or  j >= (i // C - left) * C)."""
    i = torch.arange(Tq).view(Tq, 1)
    j = torch.arange(Tk).view(1, Tk)
    vis = j < (i // chunk + 1) * chunk
    if left_chunks >= 0:
        vis = vis & (j >= (i // chunk - left_chunks) * chunk)
    if k_len is not None:
        vis = vis.unsqueeze(0) & (j.unsqueeze(0) < torch.as_tensor(k_len).view(-1, 1, 1))
    return vis


def chunk_visible_loop(Tq, Tk, chunk, left_chunks):
    """The same mask by a loop over the chunks (WeNet's subsequent_chunk_mask with num_left_chunks)."""
    m = torch.zeros(Tq, Tk, dtype=torch.bool)
    for i in range(Tq):
        start = 0 if left_chunks < 0 else max((i // chunk - left_chunks) * chunk, 0)
        end = min((i // chunk + 1) * chunk, Tk)
        m[i, start:end] = True
    return m


def sdpa_chunk_ref(q, k, v, klen, chunk, left_chunks, scale):
    """q (B, Tq, H, dk), k / v (B, Tk, H, dk), dense with autograd.  A query with no visible key: output 0 (lse 0, the kernels' value)."""
    B, Tq, H, dk = q.shape
    Tk = k.shape[1]
    vis = chunk_visible(Tq, Tk, chunk, left_chunks, klen).unsqueeze(1)       # (B, 1, Tq, Tk)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    dead = ~vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis & ~dead, float("-inf"))
    p = torch.softmax(s, -1) * (~dead).to(s.dtype)
    lse = torch.logsumexp(s, -1).masked_fill(dead.squeeze(-1), 0.0)
    return torch.einsum("bhqk,bkhd->bqhd", p, v), lse, vis


def encoder_forward(sd, cfg, wave, wave_len, chunk, left_chunks):
    """oracle.ref_model.encoder_forward with the chunk mask added to the key-padding mask (chunk <= 0: full attention)."""
    B, T, _ = wave.shape
    keep = R.valid_mask(wave_len, T)
    non_pad = keep.unsqueeze(-1).to(wave.dtype)
    masked = (~keep).unsqueeze(1).expand(B, T, T)
    if chunk > 0:
        masked = masked | ~chunk_visible(T, T, chunk, left_chunks).unsqueeze(0)
    d = cfg.d_model
    x = F.linear(wave, sd["encoder.linear_in.weight"], sd["encoder.linear_in.bias"])
    x = F.layer_norm(x, (d,), sd["encoder.layer_norm_in.weight"], sd["encoder.layer_norm_in.bias"], R.LN_EPS)
    x = x + R.positional_encoding(T, d, wave.dtype).unsqueeze(0)
    for i in range(cfg.layer_num):
        pre = f"encoder.layer_stack.{i}."
        x = R.multi_head_attention(sd, pre + "slf_attn.", x, x, masked, cfg.num_head, cfg.hidden_size) * non_pad
        x = R.feed_forward(sd, pre + "pos_ffn.", x) * non_pad
    return x


def forward_losses(sd, cfg, batch, chunk, left_chunks):
    """oracle.ref_model.forward_losses over the chunk-masked encoder."""
    out = {}
    enc = encoder_forward(sd, cfg, batch["wave"], batch["wave_len"], chunk, left_chunks)
    out["enc_out"] = enc
    loss = 0.0
    lam = float(cfg.ctc_weight)
    if cfg.use_decoder:
        cross_len = batch["tgt_len"] if cfg.cross_mask == "ref_compat" else batch["wave_len"]
        pred, gold = R.decoder_forward(sd, cfg, batch["tgt_for_input"], enc, cross_len)
        out["ce"] = R.ce_loss(pred, gold)
        loss = (1.0 - lam) * out["ce"] if lam > 0 else out["ce"]
    if lam > 0 or not cfg.use_decoder:
        logits = R.ctc_logits(sd, enc)
        out["ctc_logits"] = logits
        out["ctc"] = R.ctc_loss(logits, batch["wave_len"], batch["tgt_for_input"], batch["tgt_len"])
        loss = loss + (lam * out["ctc"] if cfg.use_decoder else out["ctc"])
    out["loss"] = loss
    return out


def loss_and_grads(sd, cfg, batch, chunk, left_chunks):
    """(loss, {name: gradient}) of one training step under the chunk mask, as RefTrainer.loss_and_grads."""
    trainable = [k for k in sd if not k.endswith("positional_encoding.pe") and k != "decoder.tgt_word_prj.weight"]
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in trainable}
    s = dict(sd)
    s.update(leaves)
    if "decoder.tgt_word_emb.weight" in leaves:
        s["decoder.tgt_word_prj.weight"] = leaves["decoder.tgt_word_emb.weight"]
    out = forward_losses(s, cfg, batch, chunk, left_chunks)
    grads = torch.autograd.grad(out["loss"], [leaves[k] for k in trainable], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(trainable, grads)}
    return out, grads
