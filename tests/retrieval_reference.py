"""The yardstick of the retrieval tests: pretreatment/clip_retrieval.py's `load` (:105-110, :175-176) and `run` (:47-83)
restated in our own words, in float64 from the fp32 inputs, with this project's tie rule (score descending, index ascending)
where the reference's unstable sort leaves equal scores open."""
import numpy as np

# Two fp32 scores of unit vectors may legitimately swap where their float64 scores differ by less than TAU(D): the fp32
# dot-product bound D 2^-24 |q| |t| for each of the two scores, doubled for the roundings of the two normalisations.
def tau(D: int) -> float:
    return 4.0 * D * 2.0 ** -24


def unit_rows64(x):
    """[M, D] -> float64 rows divided by their L2 norm (:176)."""
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def query64(frames):
    """[B, n, D] frame features -> [B, D] float64: the frame mean, L2-normalised (:105-110, :175)."""
    return unit_rows64(np.asarray(frames, dtype=np.float64).mean(1))


def scores64(q, bank_unit):
    """One query [D] against unit rows [M, D]: a row's score depends on the row alone (equal rows score equally)."""
    return (bank_unit * q[None, :]).sum(-1)


def walk(order, topk, info=None, groups=None):
    """`run`'s loop over the columns in ranked order: skip the clip's own range, skip a caption group already taken, stop at
    topk.  groups: a group id per ORIGINAL index (None: no `unique`)."""
    taken, out = set(), []
    for ind in order:
        ind = int(ind)
        if info is not None and info[0] <= ind < info[1]:
            continue
        if groups is not None:
            if groups[ind] in taken:
                continue
            taken.add(groups[ind])
        out.append(ind)
        if len(out) == topk:
            break
    return out


def ranked(scores, index):
    """`index` ordered by (score descending, index ascending)."""
    index = np.asarray(index)
    return index[np.lexsort((index, -np.asarray(scores)))]


def retrieve(q, bank_unit, topk, info=None, groups=None, sampled=None):
    """Ids (original numbering) for one unit query [D] over unit rows [M, D] (all of them, or the rows `sampled`)."""
    index = np.arange(bank_unit.shape[0]) if sampled is None else np.asarray(sampled)
    return walk(ranked(scores64(q, bank_unit[index]), index), topk, info, groups)


def retrieve_batch(image_feats, text_embs, topk, own_ranges=None, groups=None, sampled=None):
    """[B, n, D] frames and the un-normalised bank [M, D] -> a list of B id lists (each min(topk, eligible) long)."""
    q, unit = query64(image_feats), unit_rows64(text_embs)
    return [retrieve(q[b], unit, topk, None if own_ranges is None else own_ranges[b], groups, sampled) for b in range(q.shape[0])]


def group_ids(captions):
    """A group id per caption: equal strings share one."""
    seen = {}
    return np.array([seen.setdefault(c, len(seen)) for c in captions], dtype=np.int64)
