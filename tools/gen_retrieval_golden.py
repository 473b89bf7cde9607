"""Record tests/golden/retrieval/*.npz: the genuine reference's retrieved ids on small planted banks (CPU).

    python tools/gen_retrieval_golden.py

Imports pretreatment/clip_retrieval.py's own `run` (through oracle.ref_import's path handling; `clip` and `h5py`, which the
module imports and `run` never touches, are absent here and replaced by empty stand-in modules) and calls it the way its
`__main__` does (:305-321) on features normalised the way `load` does (:175-176).  Stores DATA only, per case: the fp32
inputs (frame features, the un-normalised bank), `info`, a caption-group id per bank row, `sampled_indices`, topk and the ids
`run` returned (padded with -1).

The banks are planted so that the reference's own fp32 ordering is unambiguous: the queries q_b are orthonormal, and the rows
planted for q_b are a_j q_b + sqrt(1 - a_j^2) n_j with n_j orthogonal to every query and a_j stepping down by 0.01 as the
index goes up; every other row is orthogonal to every query.  Rows of one caption group have different a_j, the lowest index
the highest: the reference's pick (the best-scoring admissible member) and this project's (the lowest admissible index) are
the same column.  tests/test_retrieval_cpu.py holds tests/retrieval_reference.py to these files.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "retrieval")
D, N_FRAMES = 64, 4


def import_run():
    from oracle import ref_import

    if not ref_import.reference_available():
        raise RuntimeError("reference tree not found at {}".format(ref_import.REFERENCE_ROOT))
    ref_import._stub_modules()
    for name in ("clip", "h5py"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    # dataloader.py and misc/ import further third-party packages at module level (a downloader, tokenisers ...) that `run`
    # never touches either: whichever of them is absent gets an empty stand-in too - never a module of the reference itself
    for _ in range(32):
        try:
            from pretreatment.clip_retrieval import run
            return run
        except ModuleNotFoundError as e:
            top = e.name.split(".")[0]
            if os.path.exists(os.path.join(ref_import.REFERENCE_ROOT, top)) or os.path.exists(os.path.join(ref_import.REFERENCE_ROOT, top + ".py")):
                raise
            print("stand-in module for the absent package `{}`".format(e.name))
            sys.modules[e.name] = types.ModuleType(e.name)
    raise RuntimeError("too many absent packages")


def planted(seed, B, M, per_query, a0=0.95):
    """(frames [B, n, D], text_embs [M, D], ranks): ranks[b] = the indices of the rows planted for query b, best first."""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((D, D)))[0].T            # orthonormal rows: B queries, D - B noise directions
    queries, noise_dirs = basis[:B], basis[B:]

    def noise():
        v = rng.standard_normal(D - B) @ noise_dirs
        return v / np.linalg.norm(v)

    rows = np.stack([noise() for _ in range(M)])
    where = rng.permutation(M)[: B * per_query].reshape(B, per_query)
    ranks = []
    for b in range(B):
        pos = np.sort(where[b])
        for r, j in enumerate(pos):
            a = a0 - 0.01 * r
            rows[j] = a * queries[b] + np.sqrt(1 - a * a) * noise()
        ranks.append(pos)
    rows *= rng.uniform(0.5, 8.0, size=(M, 1))                           # the encoder's rows are not unit
    wobble = rng.standard_normal((B, N_FRAMES, D)) * 0.05
    wobble -= wobble.mean(1, keepdims=True)                              # the frame mean stays along q_b
    frames = queries[:, None, :] * rng.uniform(2.0, 5.0, size=(B, 1, 1)) + wobble
    return frames.astype(np.float32), rows.astype(np.float32), ranks


def cases():
    B, M, P = 3, 300, 60
    frames, embs, ranks = planted(1, B, M, P)
    yield "plain", dict(frames=frames, embs=embs, topk=20)

    frames, embs, ranks = planted(2, B, M, P)
    # every clip's own range starts at its 2nd best row and is 25 wide; the last clip has none, as a video outside the bank
    info = np.array([[ranks[b][1], ranks[b][1] + 25] for b in range(B)], dtype=np.int64)
    info[B - 1] = (10 ** 9, 10 ** 9)
    yield "info", dict(frames=frames, embs=embs, topk=20, info=info)

    frames, embs, ranks = planted(3, B, M, P)
    info = np.array([[ranks[b][1], ranks[b][3] + 1] for b in range(B)], dtype=np.int64)   # covers the ranks 1, 2, 3
    groups = np.arange(M, dtype=np.int64)
    for b in range(B):
        r = ranks[b]
        groups[r[[5, 9]]] = groups[r[0]]          # all members outside the own range
        groups[r[6]] = groups[r[2]]               # the lowest member inside it, one outside
        groups[r[3]] = groups[r[1]]               # wholly inside
        groups[r[[8, 30]]] = groups[r[7]]
    background = np.setdiff1d(np.arange(M), np.concatenate(ranks))
    groups[background[:40]] = groups[background[0]]                      # one string many times, never near the top
    yield "unique", dict(frames=frames, embs=embs, topk=20, info=info, groups=groups)

    frames, embs, ranks = planted(4, B, M, P)
    info = np.array([[ranks[b][0], ranks[b][0] + 30] for b in range(B)], dtype=np.int64)
    sampled = np.sort(np.random.default_rng(40).permutation(M)[: int(M * 0.6)])
    yield "sampled", dict(frames=frames, embs=embs, topk=20, info=info, sampled=sampled)

    frames, embs, ranks = planted(5, 1, 30, 30)                          # every row planted: nothing ties at zero
    yield "short", dict(frames=frames, embs=embs, topk=50, info=np.array([[5, 12]], dtype=np.int64))


def main():
    run = import_run()
    os.makedirs(OUT, exist_ok=True)
    for name, c in cases():
        image_embs = torch.from_numpy(c["frames"]).mean(1)                                   # :105-110
        text_embs = torch.from_numpy(c["embs"])
        image_features = image_embs / image_embs.norm(dim=-1, keepdim=True)                  # :175
        text_features = text_embs / text_embs.norm(dim=-1, keepdim=True)                     # :176
        groups, info, sampled = c.get("groups"), c.get("info"), c.get("sampled")
        refs = ["caption {}".format(g) for g in groups] if groups is not None else None
        ids = np.full((c["frames"].shape[0], c["topk"]), -1, dtype=np.int64)
        for i in range(c["frames"].shape[0]):
            got = run(image_features[i, :].unsqueeze(0), text_features, topk=c["topk"],
                      info=tuple(int(v) for v in info[i]) if info is not None else None,
                      unique=groups is not None, refs=refs, sampled_indices=sampled)
            ids[i, : len(got)] = [int(v) for v in got]
        out = {"image_feats": c["frames"], "text_embs": c["embs"], "topk": np.int64(c["topk"]), "ids": ids}
        for key, val in (("info", info), ("groups", groups), ("sampled_indices", sampled)):
            if val is not None:
                out[key] = val
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("{:8s} B {} M {:3d} topk {:2d} returned {} {} bytes".format(
            name, ids.shape[0], c["embs"].shape[0], c["topk"], [int((row >= 0).sum()) for row in ids], os.path.getsize(path)))


if __name__ == "__main__":
    main()
