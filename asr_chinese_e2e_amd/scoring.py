"""Token-level scoring of hypotheses against references: the Levenshtein alignment with its split into correct tokens, substitutions,
deletions and insertions (asr_edit_align, csrc/score.hip; the definition is tests/score_ref.py), corpus CER / SER, the oracle CER of
n-best lists, per-token tallies and confusion pairs.

align_ids is the device half (one upload, one launch, one copy back); Scorer accumulates results on the host, and Scorer.add_aligned
takes results that already exist, so the accumulation does not need a GPU.  The figure the training log prints (asr_cer: edit distance
over the space-joined strings, spaces counted) is a different one; summary() reports it beside the token-level CER as
"cer_ref_convention"."""
import json

import numpy as np

from .Utils.score import calculate_cer

COR, SUB, DEL, INS = 0, 1, 2, 3      # ASR_EDIT_COR .. ASR_EDIT_INS of include/asr_hip.h
OP_NAMES = ("=", "S", "D", "I")
PAD_ID, SOS_ID, EOS_ID = 0, 2, 3     # the vocabulary's id contract (data_handler/vocab.py)


def _pack_rows(rows, width):
    out = np.zeros((len(rows), width), dtype=np.int32)
    for i, r in enumerate(rows):
        if len(r):
            out[i, :len(r)] = np.asarray(r, dtype=np.int64).astype(np.int32)
    return out


def align_ids(hyps, refs, ref_of=None, ops=True, device="cuda"):
    """hyps: P id lists, refs: R id lists, ref_of: for each hypothesis the index of its reference (None: hypothesis p against reference p,
    P == R).  Returns one dict per pair, {"distance", "cor", "sub", "del", "ins", "ops": [(op, ref_pos, hyp_pos), ...]} with op in COR /
    SUB / DEL / INS, ref_pos -1 for an insertion and hyp_pos -1 for a deletion ("ops" is left out with ops=False, which stores no
    directions on the device).  Ids are compared, never looked up: any int32 value is legal."""
    import torch

    from . import kernels as K
    P, R = len(hyps), len(refs)
    if ref_of is None:
        if P != R:
            raise ValueError(f"align_ids: {P} hypotheses for {R} references need a ref_of")
        ref_of = range(P)
    ref_of = np.asarray(list(ref_of), dtype=np.int64).reshape(-1)
    if ref_of.shape[0] != P:
        raise ValueError(f"align_ids: ref_of names {ref_of.shape[0]} references for {P} hypotheses")
    if P == 0:
        return []
    if R == 0 or ref_of.min() < 0 or ref_of.max() >= R:
        raise ValueError(f"align_ids: ref_of must lie in [0, {R})")
    hl = np.asarray([len(h) for h in hyps], dtype=np.int32)
    rl = np.asarray([len(r) for r in refs], dtype=np.int32)
    ro = ref_of.astype(np.int32)
    Lh, Lr = int(hl.max()), int(rl.max())
    if Lr > K.EDIT_MAX_REF:
        raise ValueError(f"align_ids: a reference of {Lr} tokens, the limit is {K.EDIT_MAX_REF}")
    host = np.concatenate((hl, rl, ro, _pack_rows(hyps, Lh).reshape(-1), _pack_rows(refs, Lr).reshape(-1)))
    buf = torch.from_numpy(host).to(device)      # the one upload
    o = [0, P, P + R, 2 * P + R, 2 * P + R + P * Lh]
    d_hl, d_rl, d_ro = buf[o[0]:o[1]], buf[o[1]:o[2]], buf[o[2]:o[3]]
    d_hyp, d_ref = buf[o[3]:o[4]].view(P, Lh), buf[o[4]:].view(R, Lr)
    ldo = max(Lh + Lr, 1)
    out = torch.empty(P * 6 + (P * 3 * ldo if ops else 0), dtype=torch.int32, device=buf.device)
    counts, n_ops = out[:P * 5].view(P, 5), out[P * 5:P * 6]
    ops_out = out[P * 6:].view(P, 3, ldo) if ops else None
    K.edit_align(d_hyp, d_hl, d_ref, d_rl, d_ro, hl, rl, ro, ops=ops, counts=counts, ops_out=ops_out, n_ops=n_ops if ops else None)
    got = out.cpu().numpy()                      # the one copy back
    cnt = got[:P * 5].reshape(P, 5).tolist()
    res = [{"distance": c[0], "cor": c[1], "sub": c[2], "del": c[3], "ins": c[4]} for c in cnt]
    if ops:
        k = got[P * 5:P * 6].tolist()
        planes = got[P * 6:].reshape(P, 3, ldo)
        for p in range(P):
            if k[p] < 0:
                raise RuntimeError(f"align_ids: pair {p} was not aligned (the device lengths differ from the host's)")
            res[p]["ops"] = list(zip(*planes[p, :, :k[p]].tolist())) if k[p] else []
    return res


def _is_nbest(h):
    return len(h) > 0 and isinstance(h[0], (list, tuple, np.ndarray))


class Scorer:
    """Accumulates token-level scores over a test set.  vocab: a data_handler.Vocab or a list of token strings (for the reports);
    ignore_ids are removed from hypotheses and references before anything is counted, as PAD, sos and eos always are."""

    def __init__(self, vocab, ignore_ids=()):
        self.id2token = list(vocab._id2token) if hasattr(vocab, "_id2token") else list(vocab)
        self.drop = frozenset((PAD_ID, SOS_ID, EOS_ID)) | frozenset(int(i) for i in ignore_ids)
        self.utts = []           # {"key", "ref", "hyp", "distance", "cor", "sub", "del", "ins", "ops"}
        self.oracle = []         # per n-best utterance (best distance, its rank, ranks)
        self.ref_conv = []       # the string-convention CER of each utterance's 1-best
        self.consensus = []      # per utterance scored with n-best scores (MBR distance, consensus distance, the MBR entry's rank, ranks)

    def _clean(self, ids):
        return [int(i) for i in ids if int(i) not in self.drop]

    def token(self, i):
        return self.id2token[i] if 0 <= i < len(self.id2token) else f"<{i}>"

    def _string(self, ids):
        return " ".join(self.token(i) for i in ids)

    def add(self, keys, hyps, refs, device="cuda", scores=None, posterior_scale=1.0):
        """One hypothesis (an id list) or an n-best list (a list of id lists, best first) per utterance; refs: one id list each.  An n-best
        list is aligned with ops for rank 0 and counts only for the other ranks: two launches.
        scores (one list of log-scores per utterance, entry for entry with its n-best list): the lists also go through
        consensus.consensus_ids with nbest_weights(scores, posterior_scale), and the minimum-Bayes-risk entry and the consensus string of
        each are aligned against the reference, counts only (one more launch of the same kernel): summary() then has mbr_cer,
        consensus_cer and mbr_rank_hist."""
        if not (len(keys) == len(hyps) == len(refs)):
            raise ValueError(f"Scorer.add: {len(keys)} keys, {len(hyps)} hypotheses, {len(refs)} references")
        if scores is not None:
            self._add_with_consensus(keys, hyps, refs, device, scores, posterior_scale)
            return
        nbest = any(_is_nbest(h) for h in hyps)
        lists = [[self._clean(x) for x in h] if _is_nbest(h) else [self._clean(h)] for h in hyps]
        gold = [self._clean(r) for r in refs]
        first = align_ids([l[0] for l in lists], gold, ops=True, device=device)
        rest = [(u, x) for u, l in enumerate(lists) for x in l[1:]]
        more = align_ids([x for _, x in rest], gold, ref_of=[u for u, _ in rest], ops=False, device=device) if rest else []
        results = [[r] for r in first]
        for (u, _), r in zip(rest, more):
            results[u].append(r)
        self.add_aligned(keys, results if nbest else first, hyps, refs)

    def _add_with_consensus(self, keys, hyps, refs, device, scores, posterior_scale):
        from .consensus import consensus_ids
        if not keys:
            return
        if len(scores) != len(hyps) or not all(_is_nbest(h) and len(s) == len(h) for h, s in zip(hyps, scores)):
            raise ValueError("Scorer.add: scores need an n-best list for every utterance, and one score per entry")
        lists = [[self._clean(x) for x in h] for h in hyps]
        gold = [self._clean(r) for r in refs]
        first = align_ids([l[0] for l in lists], gold, ops=True, device=device)
        cons = consensus_ids(lists, scores=scores, scale=posterior_scale, alts=1, device=device)
        rest = [(u, x) for u, l in enumerate(lists) for x in l[1:]]
        U = len(lists)
        tail = [c["mbr"] for c in cons] + [c["consensus"] for c in cons]
        more = align_ids([x for _, x in rest] + tail, gold, ref_of=[u for u, _ in rest] + 2 * list(range(U)), ops=False, device=device)
        results = [[r] for r in first]
        for (u, _), r in zip(rest, more):
            results[u].append(r)
        extra = [{"mbr_rank": c["pivot"], "mbr": more[len(rest) + u], "consensus": more[len(rest) + U + u]} for u, c in enumerate(cons)]
        self.add_aligned(keys, results, hyps, refs, consensus=extra)

    def add_aligned(self, keys, results, hyps, refs, consensus=None):
        """The host half of add: results[u] is the alignment dict of utterance u's hypothesis (score_ref.align's or align_ids'), or for an
        n-best list one dict per rank, of which rank 0 carries "ops".  hyps / refs as add takes them; positions in the ops index the ids
        that are left after ignore_ids, PAD, sos and eos are removed.
        consensus[u] (n-best lists only): {"mbr_rank", "mbr": the alignment dict of the minimum-Bayes-risk entry against the reference,
        "consensus": that of the consensus string}; only their distances are kept."""
        if not (len(keys) == len(hyps) == len(refs) == len(results)):
            raise ValueError(f"Scorer.add_aligned: {len(keys)} keys, {len(results)} results, {len(hyps)} hypotheses, {len(refs)} references")
        if consensus is not None:
            if len(consensus) != len(results) or not all(isinstance(r, (list, tuple)) for r in results):
                raise ValueError("Scorer.add_aligned: consensus needs an n-best result and one entry for every utterance")
            for c, res in zip(consensus, results):
                if not 0 <= int(c["mbr_rank"]) < len(res):
                    raise ValueError(f"Scorer.add_aligned: mbr_rank {c['mbr_rank']} outside a list of {len(res)}")
                self.consensus.append((int(c["mbr"]["distance"]), int(c["consensus"]["distance"]), int(c["mbr_rank"]), len(res)))
        for key, res, h, r in zip(keys, results, hyps, refs):
            ranks = list(res) if isinstance(res, (list, tuple)) else None
            best = ranks[0] if ranks is not None else res
            hyp = self._clean(h[0] if _is_nbest(h) else h)
            ref = self._clean(r)
            if best["cor"] + best["sub"] + best["del"] != len(ref) or best["cor"] + best["sub"] + best["ins"] != len(hyp):
                raise ValueError(f"Scorer.add_aligned: the result of {key!r} does not belong to its {len(ref)} reference and {len(hyp)} hypothesis tokens")
            self.utts.append({"key": key, "ref": ref, "hyp": hyp, "distance": int(best["distance"]), "cor": int(best["cor"]), "sub": int(best["sub"]),
                              "del": int(best["del"]), "ins": int(best["ins"]), "ops": [tuple(int(v) for v in o) for o in best["ops"]]})
            self.ref_conv.append(calculate_cer(self._string(hyp), self._string(ref)))
            if ranks is not None:
                d = [int(x["distance"]) for x in ranks]
                self.oracle.append((min(d), d.index(min(d)), len(d)))      # index: the first rank wins ties

    def summary(self):
        n = len(self.utts)
        tot = {k: sum(u[k] for u in self.utts) for k in ("cor", "sub", "del", "ins")}
        ref_tokens = sum(len(u["ref"]) for u in self.utts)
        err = tot["sub"] + tot["del"] + tot["ins"]
        out = {"utterances": n, "ref_tokens": ref_tokens, **tot,
               "cer": err / ref_tokens if ref_tokens else (float("inf") if err else 0.0),
               "ser": sum(1 for u in self.utts if u["distance"] > 0) / n if n else 0.0,
               "empty_refs": sum(1 for u in self.utts if not u["ref"]),
               "cer_ref_convention": sum(self.ref_conv) / n if n else 0.0}
        if self.oracle:
            if len(self.oracle) != n:
                raise ValueError("oracle_cer needs an n-best list for every utterance that was added")
            best = sum(o[0] for o in self.oracle)
            hist = np.bincount(np.asarray([o[1] for o in self.oracle], dtype=np.int64), minlength=max(o[2] for o in self.oracle))
            out["oracle_cer"] = best / ref_tokens if ref_tokens else (float("inf") if best else 0.0)
            out["oracle_rank_hist"] = hist.tolist()
        if self.consensus:
            if len(self.consensus) != n:
                raise ValueError("mbr_cer and consensus_cer need n-best scores for every utterance that was added")
            mbr, cons = sum(c[0] for c in self.consensus), sum(c[1] for c in self.consensus)
            hist = np.bincount(np.asarray([c[2] for c in self.consensus], dtype=np.int64), minlength=max(c[3] for c in self.consensus))
            out["mbr_cer"] = mbr / ref_tokens if ref_tokens else (float("inf") if mbr else 0.0)
            out["consensus_cer"] = cons / ref_tokens if ref_tokens else (float("inf") if cons else 0.0)
            out["mbr_rank_hist"] = hist.tolist()
        return out

    def _op_table(self):
        """Every op of the corpus as rows (op, ref id, hyp id), -1 where the op has none."""
        rows = [(op, u["ref"][i] if i >= 0 else -1, u["hyp"][j] if j >= 0 else -1) for u in self.utts for op, i, j in u["ops"]]
        return np.asarray(rows, dtype=np.int64).reshape(-1, 3)

    def per_token(self, top=None):
        """Per token {"id", "token", "cor", "sub", "del", "ins"}: cor / sub / del of the reference tokens, ins of the hypothesis tokens;
        the `top` tokens with most errors (sub + del + ins), ties by id."""
        t = self._op_table()
        tok = np.where(t[:, 0] == INS, t[:, 2], t[:, 1])
        ids, inv = np.unique(tok, return_inverse=True)
        tally = np.stack([np.bincount(inv[t[:, 0] == c], minlength=ids.shape[0]) for c in (COR, SUB, DEL, INS)], axis=1) if ids.shape[0] else np.zeros((0, 4), int)
        order = sorted(range(ids.shape[0]), key=lambda a: (-int(tally[a, 1:].sum()), int(ids[a])))
        return [{"id": int(ids[a]), "token": self.token(int(ids[a])), "cor": int(tally[a, 0]), "sub": int(tally[a, 1]), "del": int(tally[a, 2]),
                 "ins": int(tally[a, 3])} for a in order[:top]]

    def confusions(self, top=None):
        """The most frequent substitutions, {"ref_id", "hyp_id", "ref", "hyp", "count"}, ties by ids."""
        t = self._op_table()
        s = t[t[:, 0] == SUB][:, 1:]
        if not s.shape[0]:
            return []
        pairs, inv = np.unique(s, axis=0, return_inverse=True)
        cnt = np.bincount(inv.reshape(-1), minlength=pairs.shape[0])
        order = sorted(range(pairs.shape[0]), key=lambda a: (-int(cnt[a]), int(pairs[a, 0]), int(pairs[a, 1])))
        return [{"ref_id": int(pairs[a, 0]), "hyp_id": int(pairs[a, 1]), "ref": self.token(int(pairs[a, 0])), "hyp": self.token(int(pairs[a, 1])),
                 "count": int(cnt[a])} for a in order[:top]]

    def write_jsonl(self, path):
        """One line per utterance {"key", "ref", "hyp", "distance", "cor", "sub", "del", "ins", "ops"} with the ops spelled in tokens
        (["=", ref, hyp], ["S", ref, hyp], ["D", ref, null], ["I", null, hyp]), then one line {"summary": summary()}."""
        with open(path, "w", encoding="utf-8") as f:
            for u in self.utts:
                ops = [[OP_NAMES[op], self.token(u["ref"][i]) if i >= 0 else None, self.token(u["hyp"][j]) if j >= 0 else None] for op, i, j in u["ops"]]
                line = {"key": u["key"], "ref": self._string(u["ref"]), "hyp": self._string(u["hyp"]), "distance": u["distance"], "cor": u["cor"],
                        "sub": u["sub"], "del": u["del"], "ins": u["ins"], "ops": ops}
                f.write(json.dumps(line, ensure_ascii=False) + "\n")
            f.write(json.dumps({"summary": self.summary()}, ensure_ascii=False) + "\n")


def evaluate(model, batches, search="transcribe", nbest=1, scorer=None, consensus=False, posterior_scale=1.0, rescore=None, rescore_lm=None, **search_kwargs):
    """model.evaluate: every batch of `batches` through one of the model's searches, its hypotheses scored against the batch's gold ids
    (dec_preprocess of tgt_for_input: what cal_metrics scores against).  Returns the Scorer.  consensus=True (the n-best searches): the
    lists' scores go to Scorer.add with posterior_scale, so the summary also has mbr_cer, consensus_cer and mbr_rank_hist.
    rescore={column: w} (the n-best searches; rescore_lm: the NgramLM of a column "lm"): every list is re-ordered by rescore.rescore before
    anything is scored, so rank 0 is the rescored pick and a consensus sees the new totals as its scores."""
    import torch

    from . import kernels as K
    if search not in ("transcribe", "ctc_prefix_beam", "attention_beam"):
        raise ValueError(f"search must be 'transcribe', 'ctc_prefix_beam' or 'attention_beam' (got {search!r})")
    if int(nbest) < 1 or (search == "transcribe" and int(nbest) != 1):
        raise ValueError(f"nbest = {nbest}: at least 1, and exactly 1 with search='transcribe' (its searches return the best hypothesis)")
    if consensus:
        from .consensus import MAX_N
        if search == "transcribe":
            raise ValueError("consensus=True needs an n-best search: search='ctc_prefix_beam' or 'attention_beam'")
        if int(nbest) > MAX_N:
            raise ValueError(f"nbest = {nbest}: consensus takes lists of at most {MAX_N} entries")
        if not np.isfinite(float(posterior_scale)) or float(posterior_scale) <= 0.0:
            raise ValueError(f"posterior_scale must be finite and > 0 (got {posterior_scale})")
    if rescore is not None:
        from .rescore import _filled, rescore as rescore_lists
        if search == "transcribe":
            raise ValueError("rescore= needs an n-best search: search='ctc_prefix_beam' or 'attention_beam'")
        rescore = dict(rescore)
    scorer = Scorer(model.vocab) if scorer is None else scorer
    kw = dict(search_kwargs)
    beam = kw.pop("beam_size", 5)
    seen = len(scorer.utts)
    for pack in batches:
        prep = K.dec_preprocess(pack.tgt_for_input.contiguous(), SOS_ID, EOS_ID)
        lab, lab_len = prep[2].cpu(), prep[4].cpu().tolist()
        refs = [lab[b, :lab_len[b]].tolist() for b in range(lab.shape[0])]
        with torch.no_grad():
            if search == "transcribe":
                hyps = [r["ids"] for r in model.transcribe(pack, beam_size=beam, timestamps=False, **kw)]
            else:
                fn = model.ctc_prefix_beam_search if search == "ctc_prefix_beam" else model.beam_search
                found = fn(pack, beam, int(nbest), **kw)
                if rescore is not None:
                    found = rescore_lists(_filled(found), rescore, lm=rescore_lm, device=pack.wave.device)
                lists = [[list(h["yseq"]) for h in utt] for utt in found]
                for utt in lists:      # the attention searches spell sos ... eos
                    for i, seq in enumerate(utt):
                        seq = seq[1:] if seq and seq[0] == SOS_ID else seq
                        utt[i] = seq[:-1] if seq and seq[-1] == EOS_ID else seq
                hyps = [utt or [[]] for utt in lists] if int(nbest) > 1 or consensus else [utt[0] if utt else [] for utt in lists]
        keys = list(pack.key) if pack.get("key") is not None else [f"utt{seen + b}" for b in range(len(refs))]
        if consensus:
            scores = [[float(h["score"]) for h in utt] or [0.0] for utt in found]
            scorer.add(keys, hyps, refs, device=pack.wave.device, scores=scores, posterior_scale=posterior_scale)
        else:
            scorer.add(keys, hyps, refs, device=pack.wave.device)
        seen += len(refs)
    return scorer
