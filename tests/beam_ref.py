"""Plain-Python restatement of one merge step of the attention beam search (asr_beam_step, csrc/decode.hip), written from the
reference's Decoder.recognize_beam (Predictor/Models/transformer_official.py:331-434, restated per utterance in
oracle/ref_model.beam_search):

  * every live hypothesis h of an utterance is extended by its `beam` candidate tokens j (the best entries of its log-softmax);
    the candidate's score is score[h] + val[h][j], summed in fp32 as the kernel does;
  * the candidates, taken in (h, j) order, are ranked by Python's stable sorted(reverse=True) - equal scores keep their first-come
    order - and the best `beam` survive, in rank order, into slots 0 .. beam-1;
  * a survivor whose token is eos leaves the beam (end = 1); at the last step (step == maxlen[b] - 1) eos is appended to every
    survivor, its own eos included (end = 2); an utterance with step >= maxlen[b] has no candidates;
  * slots no candidate lands in are dead: alive 0, parent = the slot itself, a record of (token 0, parent 0, end 0, score -inf);
    their score / last token are left as they were;
  * the number of survivors that stay in the beam is ADDED onto the caller's counter.

The reference keeps the best `beam` after each hypothesis (sorted(...)[:beam] inside the loop); one stable sort of all candidates
keeps the same ones in the same order, since truncating never drops a candidate that the full sort would rank above `beam`.
tests/test_beam_ref_cpu.py pins this restatement on hand-worked cases; tests/test_decode_kernels_gpu.py checks the kernel against it.
"""
import numpy as np


def beam_step(top_vals, top_ids, score, alive, last_tok, maxlen, step, eos):
    """One step for B utterances.  top_vals (B, beam, beam) f32, top_ids (B, beam, beam) int, score (B, beam) f32, alive /
    last_tok (B, beam) int, maxlen (B,) int.  Returns dict(score, alive, last_tok, parent, rec_tok, rec_par, rec_end, rec_score,
    n_alive): the state after the step (arrays of the input shapes), this step's records (B, beam) and the survivor count."""
    top_vals = np.asarray(top_vals, dtype=np.float32)
    top_ids = np.asarray(top_ids)
    B, beam = top_vals.shape[0], top_vals.shape[1]
    out = dict(score=np.array(score, dtype=np.float32), alive=np.zeros((B, beam), np.int32), last_tok=np.array(last_tok, dtype=np.int32),
               parent=np.tile(np.arange(beam, dtype=np.int32), (B, 1)), rec_tok=np.zeros((B, beam), np.int32),
               rec_par=np.zeros((B, beam), np.int32), rec_end=np.zeros((B, beam), np.int32),
               rec_score=np.full((B, beam), -np.inf, np.float32), n_alive=0)
    for b in range(B):
        if step >= int(maxlen[b]):
            continue
        cands = []
        for h in range(beam):
            if not alive[b][h]:
                continue
            for j in range(beam):
                s = np.float32(score[b][h]) + top_vals[b, h, j]          # fp32 sum
                cands.append((float(s), h, int(top_ids[b, h, j])))
        kept = sorted(cands, key=lambda c: c[0], reverse=True)[:beam]
        last = step == int(maxlen[b]) - 1
        for k, (s, h, tok) in enumerate(kept):
            end = 2 if last else (1 if tok == eos else 0)
            out["score"][b, k] = s
            out["last_tok"][b, k] = tok
            out["parent"][b, k] = h
            out["alive"][b, k] = 0 if end else 1
            out["rec_tok"][b, k], out["rec_par"][b, k], out["rec_end"][b, k], out["rec_score"][b, k] = tok, h, end, s
            out["n_alive"] += 0 if end else 1
    return out
