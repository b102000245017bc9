"""Rescoring of n-best lists: re-rank the lists a search returns with a weighted sum of scores, and find the weights on a dev set
(asr_lm_score_nbest and asr_nbest_sweep, csrc/rescore.hip; the definition is tests/rescore_ref.py).

An entry of a list has K <= 8 features, each finite or -inf: the scores the search reports (ctc_score, att_score, bias, lm_score, score),
"lm" - the n-gram LM score of the finished string, computed here for all entries in one launch - and "len", its token count.  Its total
under a weight vector w is  total = 0.0; for k ascending: if w[k] != 0.0: total = total + (w[k] * f[k])  - a rounded product, then a
rounded sum, a zero weight's term skipped.  An entry with a non-finite feature under a non-zero weight is unscorable.  The pick is the
scorable entry of greatest total, the lowest index on ties.  No search is changed or run again: the LM's weight is a column weight, not
folded into the LM's tables, so one pass over a dev set gives the error counts of every point of a grid (sweep, SweepResult).

lm_scores is one upload, one launch and one copy back; sweep is the edit kernel (counts only) over all entries, then the sweep kernel."""
import itertools
import json
import math

import numpy as np

MAX_N, MAX_K, MAX_G = 64, 8, 65536      # ASR_RESCORE_MAX_* of include/asr_hip.h
SCORE_COLUMNS = ("ctc_score", "att_score", "bias")


# ------------------------------------------------------------------------------------------------ the LM score of many finished strings
def _token_rows(lists, what):
    """(tok (P, L) int32, len (P) int32, sizes) of U lists of id lists in list order; a None entry is absent (-1)."""
    if len(lists) == 0:
        raise ValueError(f"{what}: no lists")
    flat = [h for l in lists for h in l]
    if not flat:
        raise ValueError(f"{what}: no entries")
    L = max((len(h) for h in flat if h is not None), default=0)
    tok, ln = np.zeros((len(flat), L), dtype=np.int32), np.full(len(flat), -1, dtype=np.int32)
    for p, h in enumerate(flat):
        if h is None:
            continue
        ids = np.asarray(h, dtype=np.int64).reshape(-1)
        if ids.shape[0] and (ids.min() < -2 ** 31 or ids.max() > 2 ** 31 - 1):
            raise ValueError(f"{what}: entry {p} has an id outside int32")
        ln[p] = ids.shape[0]
        tok[p, :ids.shape[0]] = ids
    return tok, ln, [len(l) for l in lists]


def lm_scores(lists, lm, device="cuda"):
    """lists: per utterance a list of id lists, None = absent.  Returns per utterance a list of {"lm_score" (lm.score of the string),
    "bias", "state" (lm.walk), "tokens"} - bit for bit the host methods' values; an absent entry gives (0.0, 0.0, -1, 0).  One upload,
    one launch (asr_lm_score_nbest), one copy back."""
    import torch

    from . import kernels as K
    tok, ln, sizes = _token_rows(lists, "lm_scores")
    P, L = tok.shape
    buf = torch.from_numpy(np.concatenate((ln, tok.reshape(-1)))).to(device)      # the one upload
    out = torch.empty(6 * P, dtype=torch.int32, device=buf.device)
    K.lm_score_nbest(buf[P:].view(P, L), buf[:P], ln, lm, out=out)
    got = out.cpu().numpy()                                                        # the one copy back
    score, bias = got[:2 * P].view(np.float64).tolist(), got[2 * P:4 * P].view(np.float64).tolist()
    state, ntok = got[4 * P:5 * P].tolist(), got[5 * P:].tolist()
    rows = [{"lm_score": score[p], "bias": bias[p], "state": state[p], "tokens": ntok[p]} for p in range(P)]
    at = np.cumsum([0] + sizes).tolist()
    return [rows[at[u]:at[u + 1]] for u in range(len(sizes))]


def lm_scores_packed(tok, ln, lm, host_len=None):
    """The same for lists that are on the device already, in the searches' layout: tok (..., L) int32 with unit stride along L and equal
    row distances, ln (...) int32 (-1 = absent).  host_len: ln on the host (it is copied back when not given: the launcher refuses by
    it).  Returns device tensors {"lm_score", "bias" float64, "state", "tokens" int32} of ln's shape: views of one buffer ("buffer")."""
    from . import kernels as K
    shape = tuple(ln.shape)
    L = tok.shape[-1]
    rows = tok.reshape(-1, L)
    if rows.data_ptr() != tok.data_ptr():
        raise ValueError("lm_scores_packed: the rows of tok must be equally spaced (a contiguous tensor, or a view with one row stride)")
    flat = ln.reshape(-1)
    hl = flat.cpu().numpy() if host_len is None else np.asarray(host_len, dtype=np.int32).reshape(-1)
    score, bias, state, ntok = K.lm_score_nbest(rows, flat.contiguous(), hl, lm)
    out = {"lm_score": score.view(shape), "bias": bias.view(shape), "state": state.view(shape), "tokens": ntok.view(shape)}
    out["buffer"] = score._base if score._base is not None else score
    return out


# ------------------------------------------------------------------------------------------------ features of what a search returned
def _strip(seq, sos, eos):
    seq = [int(x) for x in seq]
    seq = seq[1:] if seq and seq[0] == sos else seq
    return seq[:-1] if seq and seq[-1] == eos else seq


def _check_unit_lm(lm):
    if lm is None:
        raise ValueError("the column 'lm' needs lm=: an NgramLM.from_arpa(..., weight=1.0, ins=0.0)")
    if float(lm.weight) != 1.0 or float(lm.ins) != 0.0:
        raise ValueError(f"the column 'lm' needs an LM whose terms are natural-log probabilities, so that the swept weight means what NgramLM(weight=) means: "
                         f"compile it with NgramLM.from_arpa(..., weight=1.0, ins=0.0) (got weight={lm.weight}, ins={lm.ins})")


def check_features(f):
    """f as a (U, N, K) float64 array; raises for NaN, +inf or a shape past the limits."""
    f = np.ascontiguousarray(np.asarray(f, dtype=np.float64))
    if f.ndim != 3 or f.shape[0] < 1:
        raise ValueError(f"features: a (U, N, K) array (got shape {f.shape})")
    if not 1 <= f.shape[1] <= MAX_N:
        raise ValueError(f"features: lists of {f.shape[1]} entries (N), between 1 and {MAX_N} are taken")
    if not 1 <= f.shape[2] <= MAX_K:
        raise ValueError(f"features: {f.shape[2]} columns (K), between 1 and {MAX_K} are taken")
    if np.isnan(f).any() or (f == np.inf).any():
        raise ValueError("features: a value is NaN or +inf (finite or -inf are taken)")
    return f


def features(found, lm=None, columns=None, device="cuda"):
    """found: what a search returns - per utterance a list of dicts with "yseq", "score" and whatever of "ctc_score", "att_score", "bias",
    "lm_score" the search reports.  Returns (names, f (U, N, K) float64, lists): lists[u][e] = the entry's ids with sos / eos stripped as
    scoring.evaluate strips them, None for the entries a shorter list lacks (their features are 0.0).
    columns: names of entry keys, "lm" (lm_scores of the stripped ids; needs lm=, compiled with weight=1.0 and ins=0.0) and "len" (the
    token count).  Default: every one of ctc_score, att_score, bias that all entries carry - "score" if neither ctc_score nor att_score
    is there - and "lm" when an LM is given."""
    from .scoring import EOS_ID, SOS_ID
    U = len(found)
    if U == 0:
        raise ValueError("features: no lists")
    entries = [h for utt in found for h in utt]
    if columns is None:
        columns = [c for c in SCORE_COLUMNS if entries and all(c in h for h in entries)]
        if "ctc_score" not in columns and "att_score" not in columns:
            columns = ["score"]
        if lm is not None:
            columns.append("lm")
    names = [str(c) for c in columns]
    if not 1 <= len(names) <= MAX_K:
        raise ValueError(f"features: {len(names)} columns (K), between 1 and {MAX_K} are taken")
    if len(set(names)) != len(names):
        raise ValueError(f"features: a column is named twice in {names}")
    N = max(len(utt) for utt in found)
    if not 1 <= N <= MAX_N:
        raise ValueError(f"features: lists of {N} entries (N), between 1 and {MAX_N} are taken")
    for u, utt in enumerate(found):
        if not utt:
            raise ValueError(f"features: list {u} has no entry")
    lists = [[_strip(h["yseq"], SOS_ID, EOS_ID) for h in utt] + [None] * (N - len(utt)) for utt in found]
    lms = None
    if "lm" in names:
        _check_unit_lm(lm)
        lms = lm_scores(lists, lm, device=device)
    f = np.zeros((U, N, len(names)), dtype=np.float64)
    for u, utt in enumerate(found):
        for e, h in enumerate(utt):
            for k, c in enumerate(names):
                if c == "lm":
                    f[u, e, k] = lms[u][e]["lm_score"]
                elif c == "len":
                    f[u, e, k] = float(len(lists[u][e]))
                elif c in h:
                    f[u, e, k] = float(h[c])
                else:
                    raise ValueError(f"features: entry {e} of list {u} carries no {c!r} (it has {sorted(h)})")
    return names, check_features(f), lists


def _weight_vector(names, weights):
    extra = [c for c in weights if c not in names]
    if extra:
        raise ValueError(f"weights name {extra}, the columns are {names}")
    w = [float(weights.get(c, 0.0)) for c in names]
    if not all(math.isfinite(x) for x in w):
        raise ValueError(f"weights must be finite (got {weights})")
    return w


def _device_sweep(f, lists, err, grid, totals=False, device="cuda"):
    """asr_nbest_sweep over host arrays: f (U, N, K), lists (None = absent), err (U, N, 3) int32, grid (G, K).  One upload of each kind,
    one copy back.  Returns (pick (G, U), tot (G, 4), total (G, U, N) | None) as numpy arrays."""
    import torch

    from . import kernels as K
    f = check_features(f)
    U, N, Kc = f.shape
    grid = np.ascontiguousarray(np.asarray(grid, dtype=np.float64))
    if grid.ndim != 2 or grid.shape[1] != Kc:
        raise ValueError(f"a grid of shape {grid.shape} for {Kc} columns")
    if not 1 <= grid.shape[0] <= MAX_G:
        raise ValueError(f"a grid of {grid.shape[0]} points (G), between 1 and {MAX_G} are taken")
    if not np.isfinite(grid).all():
        raise ValueError("a grid weight is not finite")
    if len(lists) != U or any(len(l) != N for l in lists):
        raise ValueError(f"{U} x {N} features need as many list entries (None = absent)")
    present = np.asarray([[h is not None for h in l] for l in lists], dtype=bool)
    if not present.any(axis=1).all():
        raise ValueError(f"utterance {int(np.argmin(present.any(axis=1)))} has no present entry")
    hf = np.ascontiguousarray(f.transpose(2, 1, 0))                                   # (K, N, U): the one transposition
    hl = np.ascontiguousarray(np.where(present, 0, -1).astype(np.int32).T)            # (N, U)
    he = np.ascontiguousarray(np.asarray(err, dtype=np.int32).reshape(U, N, 3).transpose(2, 1, 0))      # (3, N, U)
    d_f = torch.from_numpy(np.concatenate((hf.reshape(-1), grid.reshape(-1)))).to(device)
    d_i = torch.from_numpy(np.concatenate((hl.reshape(-1), he.reshape(-1)))).to(d_f.device)
    G = grid.shape[0]
    pick, tot, total = K.nbest_sweep(d_f[:hf.size].view(Kc, N, U), d_i[:hl.size].view(N, U), d_i[hl.size:].view(3, N, U), d_f[hf.size:].view(G, Kc),
                                     hf, hl, grid, totals=totals)
    return pick.cpu().numpy(), tot.cpu().numpy(), (total.cpu().numpy() if totals else None)


def rescore(found, weights, lm=None, device="cuda"):
    """found as features takes it; weights: {column: w} (columns as features names them).  Returns the lists re-ordered: the scorable
    entries by descending total, then ascending first rank, then the unscorable ones in their order.  Every entry is a copy with "score" =
    the new total (-inf if unscorable), "first_rank" = its old index, and "lm" / "len" where those columns are used.  The totals come
    from asr_nbest_sweep with one grid point; the order is made on the host.  The input is not modified."""
    weights = dict(weights)
    names, f, lists = features(found, lm=lm, columns=list(weights), device=device)
    w = _weight_vector(names, weights)
    U, N, _ = f.shape
    _, _, total = _device_sweep(f, lists, np.zeros((U, N, 3), dtype=np.int32), [w], totals=True, device=device)
    out = []
    for u, utt in enumerate(found):
        t = total[0, u].tolist()
        order = sorted(range(len(utt)), key=lambda e: (t[e] == -math.inf, -t[e] if t[e] != -math.inf else 0.0, e))
        new = []
        for e in order:
            h = dict(utt[e])
            h["score"], h["first_rank"] = t[e], e
            for k, c in enumerate(names):
                if c in ("lm", "len"):
                    h[c] = float(f[u, e, k]) if c == "lm" else int(f[u, e, k])
            new.append(h)
        out.append(new)
    return out


# ------------------------------------------------------------------------------------------------ the grid and the sweep
def parse_axis(text):
    """`lo:hi:step` -> lo + i * step in float64 for i = 0 .. floor((hi - lo) / step + 1e-9): both ends included; `a,b,c` or `a` -> the
    listed values."""
    text = str(text).strip()
    if ":" in text:
        parts = text.split(":")
        if len(parts) != 3:
            raise ValueError(f"an axis is lo:hi:step (got {text!r})")
        lo, hi, step = (float(p) for p in parts)
        if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(step)) or step <= 0.0 or hi < lo:
            raise ValueError(f"an axis lo:hi:step needs finite values, step > 0 and hi >= lo (got {text!r})")
        q = (hi - lo) / step
        if q >= MAX_G:
            raise ValueError(f"the axis {text!r} has more than {MAX_G} points")
        return [lo + i * step for i in range(int(math.floor(q + 1e-9)) + 1)]
    vals = [float(p) for p in text.split(",") if p.strip()]
    if not vals:
        raise ValueError(f"an empty axis {text!r}")
    return vals


def parse_grid(text):
    """`att_score=1;ctc_score=0:1:0.25;lm=0:1:0.1` -> Grid, the axes in the order given."""
    axes = {}
    for part in str(text).split(";"):
        if not part.strip():
            continue
        if "=" not in part:
            raise ValueError(f"a grid axis is name=values (got {part!r})")
        name, vals = part.split("=", 1)
        if name.strip() in axes:
            raise ValueError(f"the axis {name.strip()!r} is given twice")
        axes[name.strip()] = parse_axis(vals)
    return Grid(**axes)


class Grid:
    """The Cartesian product of the axes, row-major in the order they are given: Grid(ctc_score=[1.0], att_score=[0.5, 1, 2],
    lm=np.arange(0, 1.01, 0.1)).  names: the columns; points (G, K) float64.  Grid.explicit(names, points): a list of weight vectors."""

    def __init__(self, **axes):
        if not 1 <= len(axes) <= MAX_K:
            raise ValueError(f"a grid has 1 to {MAX_K} axes (got {len(axes)})")
        vals = [np.asarray(v, dtype=np.float64).reshape(-1) for v in axes.values()]
        G = 1
        for n, v in zip(axes, vals):
            if v.shape[0] < 1 or not np.isfinite(v).all():
                raise ValueError(f"the axis {n!r} needs at least one value, all finite")
            G *= v.shape[0]
            if G > MAX_G:
                raise ValueError(f"a grid of more than {MAX_G} points (G)")
        self.names = list(axes)
        self.points = np.ascontiguousarray(np.asarray(list(itertools.product(*[v.tolist() for v in vals])), dtype=np.float64).reshape(G, len(vals)))

    @classmethod
    def explicit(cls, names, points):
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
        names = [str(n) for n in names]
        if pts.ndim != 2 or pts.shape[1] != len(names) or not 1 <= len(names) <= MAX_K or len(set(names)) != len(names):
            raise ValueError(f"Grid.explicit: points (G, K) for 1 to {MAX_K} distinct names (got shape {pts.shape} for {names})")
        if not 1 <= pts.shape[0] <= MAX_G:
            raise ValueError(f"a grid of {pts.shape[0]} points (G), between 1 and {MAX_G} are taken")
        if not np.isfinite(pts).all():
            raise ValueError("a grid weight is not finite")
        g = cls.__new__(cls)
        g.names, g.points = names, pts
        return g

    def __len__(self):
        return self.points.shape[0]


def _best(sub, dele, ins, wrong):
    errs = (sub + dele + ins).tolist()
    wr = wrong.tolist()
    return min(range(len(errs)), key=lambda g: (errs[g], wr[g], g))


class SweepResult:
    """The error counts of every grid point over the utterances seen so far.  names, grid (G, K), sub / del / ins / wrong (G) int64,
    ref_tokens, utterances, rank0 / oracle (the errors of the lists as given and of their best entries), pick (G, U) on request.
    cer, ser, best, best_weights, rank0_cer, oracle_cer follow from them."""

    def __init__(self, names, grid, sub, dele, ins, wrong, ref_tokens, utterances, rank0, oracle, pick=None):
        self.names, self.grid = list(names), np.asarray(grid, dtype=np.float64)
        self.sub, self.ins, self.wrong = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (sub, ins, wrong))
        setattr(self, "del", np.asarray(dele, dtype=np.int64).reshape(-1))
        self.ref_tokens, self.utterances, self.rank0, self.oracle = int(ref_tokens), int(utterances), int(rank0), int(oracle)
        self.pick = pick
        G = self.grid.shape[0]
        if self.grid.ndim != 2 or self.grid.shape[1] != len(self.names) or any(a.shape[0] != G for a in (self.sub, self.dele, self.ins, self.wrong)):
            raise ValueError("SweepResult: one count per grid point, one grid column per name")

    dele = property(lambda self: getattr(self, "del"))

    def _rate(self, errs):
        return errs / self.ref_tokens if self.ref_tokens else (math.inf if errs else 0.0)

    @property
    def cer(self):
        return np.asarray([self._rate(int(e)) for e in (self.sub + self.dele + self.ins)], dtype=np.float64)

    @property
    def ser(self):
        return self.wrong / self.utterances if self.utterances else np.zeros(self.wrong.shape[0])

    @property
    def best(self):
        return _best(self.sub, self.dele, self.ins, self.wrong)

    @property
    def best_weights(self):
        return {n: float(x) for n, x in zip(self.names, self.grid[self.best])}

    rank0_cer = property(lambda self: self._rate(self.rank0))
    oracle_cer = property(lambda self: self._rate(self.oracle))

    def add(self, other):
        """The sum of two results over the same grid (a dev set goes through batch by batch); the picks are concatenated."""
        if self.names != other.names or self.grid.shape != other.grid.shape or not np.array_equal(self.grid, other.grid):
            raise ValueError("SweepResult.add: the two results have different grids")
        pick = np.concatenate((self.pick, other.pick), axis=1) if self.pick is not None and other.pick is not None else None
        return SweepResult(self.names, self.grid, self.sub + other.sub, self.dele + other.dele, self.ins + other.ins, self.wrong + other.wrong,
                           self.ref_tokens + other.ref_tokens, self.utterances + other.utterances, self.rank0 + other.rank0, self.oracle + other.oracle, pick)

    def to_dict(self):
        b = self.best
        return {"names": self.names, "grid": self.grid.tolist(), "sub": self.sub.tolist(), "del": self.dele.tolist(), "ins": self.ins.tolist(),
                "wrong": self.wrong.tolist(), "cer": self.cer.tolist(), "ser": np.asarray(self.ser).tolist(), "ref_tokens": self.ref_tokens,
                "utterances": self.utterances, "rank0_errors": self.rank0, "oracle_errors": self.oracle, "rank0_cer": self.rank0_cer,
                "oracle_cer": self.oracle_cer, "best": b, "best_weights": self.best_weights, "best_cer": float(self.cer[b])}

    def save(self, path):
        with open(path, "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f, indent=1)
            f.write("\n")

    @classmethod
    def load(cls, path):
        with open(path, encoding="utf-8") as f:
            d = json.load(f)
        return cls(d["names"], d["grid"], d["sub"], d["del"], d["ins"], d["wrong"], d["ref_tokens"], d["utterances"], d["rank0_errors"], d["oracle_errors"])


def load_weights(path):
    """{column: w} from a file SweepResult.save wrote (its best_weights), or from a plain JSON object of weights."""
    with open(path, encoding="utf-8") as f:
        d = json.load(f)
    w = d.get("best_weights", d)
    if not isinstance(w, dict) or not w or not all(isinstance(v, (int, float)) for v in w.values()):
        raise ValueError(f"{path}: neither a saved SweepResult nor an object of column weights")
    return {str(k): float(v) for k, v in w.items()}


def _clean(ids):
    from .scoring import EOS_ID, PAD_ID, SOS_ID
    return [int(i) for i in ids if int(i) not in (PAD_ID, SOS_ID, EOS_ID)]


def entry_errors(lists, refs, device="cuda"):
    """err (U, N, 3) int32 = (sub, del, ins) of every present entry against its utterance's reference (asr_edit_align, counts only: one
    launch); zeros for absent entries.  PAD, sos and eos count nowhere, as in scoring.Scorer."""
    from .scoring import align_ids
    U, N = len(lists), max(len(l) for l in lists)
    where = [(u, e) for u, l in enumerate(lists) for e, h in enumerate(l) if h is not None]
    got = align_ids([_clean(lists[u][e]) for u, e in where], [_clean(r) for r in refs], ref_of=[u for u, _ in where], ops=False, device=device)
    err = np.zeros((U, N, 3), dtype=np.int32)
    for (u, e), r in zip(where, got):
        err[u, e] = (r["sub"], r["del"], r["ins"])
    return err


def sweep(found_or_features, refs, grid, lm=None, picks=False, device="cuda"):
    """found_or_features: what a search returned (features(found, lm, grid.names) is taken of it), or features' own result (names, f,
    lists) with names == grid.names.  refs: one id list per utterance (what the entries' stripped ids are scored against).  grid: a Grid.
    Runs asr_edit_align, counts only, over all entries, then asr_nbest_sweep.  Returns a SweepResult; picks=True keeps pick (G, U)."""
    if isinstance(found_or_features, tuple) and len(found_or_features) == 3 and not isinstance(found_or_features[0], dict):
        names, f, lists = found_or_features
        names = list(names)
        if names != list(grid.names):
            raise ValueError(f"sweep: the features' columns {names} are not the grid's {grid.names}")
    else:
        names, f, lists = features(found_or_features, lm=lm, columns=list(grid.names), device=device)
    if len(refs) != len(lists):
        raise ValueError(f"sweep: {len(refs)} references for {len(lists)} lists")
    f = check_features(f)
    N = f.shape[1]
    lists = [list(l) + [None] * (N - len(l)) for l in lists]
    err = entry_errors(lists, refs, device=device)
    pick, tot, _ = _device_sweep(f, lists, err, grid.points, device=device)
    dist = err.sum(axis=2).astype(np.int64)
    first = [next(e for e, h in enumerate(l) if h is not None) for l in lists]
    rank0 = int(sum(dist[u, e] for u, e in enumerate(first)))
    oracle = int(sum(min(dist[u, e] for e, h in enumerate(l) if h is not None) for u, l in enumerate(lists)))
    return SweepResult(names, grid.points, tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 3], sum(len(_clean(r)) for r in refs), len(lists), rank0, oracle,
                       pick if picks else None)


# ------------------------------------------------------------------------------------------------ the model
def _search(model, pack, search, beam_size, nbest, search_kwargs):
    import torch
    if search not in ("ctc_prefix_beam", "attention_beam"):
        raise ValueError(f"search must be 'ctc_prefix_beam' or 'attention_beam' (got {search!r})")
    if not 1 <= int(nbest) <= MAX_N:
        raise ValueError(f"nbest = {nbest}: between 1 and {MAX_N}")
    fn = model.ctc_prefix_beam_search if search == "ctc_prefix_beam" else model.beam_search
    with torch.no_grad():
        return fn(pack, int(beam_size), int(nbest), **search_kwargs)


def _filled(found):
    """An utterance for which the search found nothing gets the empty string, as scoring.evaluate scores it."""
    return [utt if utt else [{"yseq": [], "score": 0.0, "ctc_score": 0.0, "att_score": 0.0, "bias": 0.0, "lm_score": 0.0}] for utt in found]


def model_rescore(model, pack, weights, search="attention_beam", beam_size=5, nbest=5, lm=None, **search_kwargs):
    """model.rescore: the n-best lists of one pack through rescore."""
    found = _search(model, pack, search, beam_size, nbest, search_kwargs)
    return rescore(_filled(found), weights, lm=lm, device=pack.wave.device)


def gold_ids(pack):
    """The gold ids scoring.evaluate scores a pack against."""
    from . import kernels as K
    from .scoring import EOS_ID, SOS_ID
    prep = K.dec_preprocess(pack.tgt_for_input.contiguous(), SOS_ID, EOS_ID)
    lab, lab_len = prep[2].cpu(), prep[4].cpu().tolist()
    return [lab[b, :lab_len[b]].tolist() for b in range(lab.shape[0])]


def model_tune(model, batches, grid, search="attention_beam", beam_size=10, nbest=10, lm=None, **search_kwargs):
    """model.tune: every pack through the search once, its lists through sweep; the SweepResults are summed."""
    total = None
    for pack in batches:
        found = _filled(_search(model, pack, search, beam_size, nbest, search_kwargs))
        res = sweep(found, gold_ids(pack), grid, lm=lm, device=pack.wave.device)
        total = res if total is None else total.add(res)
    if total is None:
        raise ValueError("tune: no batches")
    return total
