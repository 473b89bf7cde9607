"""CPU: the definition of sampled decoding (tests/sample_reference.py, the float64 restatement of care_sample_logits) - the
hash against constants worked out by hand, the distribution it draws from, the tie rules - and the host side: the params
block, the Translator's refusals, the seed drawn from torch's generator."""
import math
import struct

import numpy as np
import pytest
import torch

import sample_reference as R


def test_hash_against_hand_computed_constants():
    # fin(0) = 0 (every step of the finaliser maps 0 to 0); h(0, 0) = fin(0x9E3779B97F4A7C15) is the first output of the
    # published splitmix64 generator seeded with 0
    assert R.fin(0) == 0
    assert R.h(0, 0) == 0xE220A8397B1DCDAF
    assert R.fin(1) == 0x5692161D100B05E5
    assert R.h(12345, 7) == 0x6E7411B06820371C
    assert R.row_state(2024, 3, 5) == R.h(2024, (3 << 16) | 5) == 0x93CFA83E11635B76
    assert R.h_vec(12345, np.array([7, 0], dtype=np.uint64)).tolist() == [7959005890829367068, 2454886589211414944]
    assert int(R.h_vec(0, np.array([0], dtype=np.uint64))[0]) == R.h(0, 0)
    u = R.uniforms(2024, 3, 5, 4)
    assert [float(v).hex() for v in u] == ["0x1.16e7a60000000p-1", "0x1.e76e840000000p-2", "0x1.d4718a0000000p-1", "0x1.fc3e340000000p-2"]
    # u = (2 k + 1) 2^-24 is exact in fp32, inside (0, 1), and the Gumbel term it gives is bounded: the tail beyond
    # g = -log(-log(1 - 2^-24)) = 16.64 (probability 6e-8 per entry) is cut
    big = R.uniforms(1, 2, 3, 4096)
    assert (big.astype(np.float32).astype(np.float64) == big).all() and big.min() >= 2.0 ** -24 and big.max() <= 1 - 2.0 ** -24
    assert -math.log(-math.log(1 - 2.0 ** -24)) < 16.64 and 1 - math.exp(-math.exp(-16.63)) < 6.1e-8


def test_params_block_is_the_kernels_24_bytes():
    from care_amd.engine_sample import PARAMS_BYTES, pack_params

    blk = pack_params(2 ** 63 + 5, 0.7, 20, 0.9)
    assert len(blk) == PARAMS_BYTES == 24 and blk == R.pack_params(2 ** 63 + 5, 0.7, 20, 0.9)
    seed, inv_t, top_p, top_k, reserved = struct.unpack("<Qffii", blk)
    assert (seed, top_k, reserved) == (2 ** 63 + 5, 20, 0)
    assert inv_t == float(np.float32(1.0 / 0.7)) and top_p == float(np.float32(0.9))


def _draws(x, n, seed, temperature=1.0, top_k=0, top_p=1.0, t=1):
    """The tokens of keys 0 .. n - 1 for one logit row, vectorised over the keys (the kept set does not depend on the key);
    the first 64 are checked against sample_row itself."""
    V = x.shape[0]
    first = R.sample_row(x, seed, 0, t, temperature, top_k, top_p)
    kept = np.sort(first["kept"])
    s = ((x * np.float32(1.0 / temperature)).astype(np.float32) + np.float32(0)).astype(np.float64)
    states = np.array([R.row_state(seed, k, t) for k in range(n)], dtype=np.uint64)
    kk = R.h_vec(states[:, None], np.arange(V, dtype=np.uint64)[None, :]) >> np.uint64(41)
    g = -np.log(-np.log((2.0 * kk.astype(np.float64) + 1.0) * 2.0 ** -24))
    toks = kept[np.argmax(s[kept][None, :] + g[:, kept], axis=1)]
    assert toks[:64].tolist() == [R.sample_row(x, seed, k, t, temperature, top_k, top_p)["tok"] for k in range(64)]
    return toks, first


def _chi_square(toks, probs):
    n = toks.shape[0]
    counts = np.bincount(toks, minlength=probs.shape[0]).astype(np.float64)
    assert (counts[probs == 0] == 0).all()
    live = probs > 0
    return float((((counts - n * probs) ** 2)[live] / (n * probs[live])).sum())


@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 12, 1.0), (1.0, 0, 0.8), (1.3, 20, 0.9)])
def test_draws_follow_the_filtered_softmax(temperature, top_k, top_p):
    """20 000 draws over distinct keys from a 37-entry row: chi-square against the renormalised softmax of the kept set under
    70 (36 degrees of freedom at most: the 99.9 % point is 68)."""
    x = np.random.default_rng(37).standard_normal(37).astype(np.float32)
    toks, first = _draws(x, 20000, seed=99, temperature=temperature, top_k=top_k, top_p=top_p)
    s = (x * np.float32(1.0 / temperature)).astype(np.float64)
    probs = np.zeros(37)
    probs[first["kept"]] = np.exp(s[first["kept"]] - s.max())
    probs /= probs.sum()
    if top_k:
        assert first["nkept"] <= top_k
    if top_k and top_p == 1.0:
        assert sorted(first["kept"].tolist()) == sorted(np.argsort(-s, kind="stable")[:top_k].tolist())
    if top_p < 1.0:   # the smallest prefix whose mass reaches top_p (within what top-k left)
        order = first["kept"]
        base = np.sort(np.exp(s - s.max()))[::-1][: top_k or 37]
        mass = np.cumsum(np.exp(s[order] - s.max())) / base.sum()
        assert mass[-1] >= np.float32(top_p) and (order.size == 1 or mass[-2] < np.float32(top_p))
    chi = _chi_square(toks, probs)
    print("chi-square", temperature, top_k, top_p, first["nkept"], chi)
    assert chi < 70


def test_top_k_1_is_the_argmax_and_a_tiny_top_p_keeps_one_entry():
    rng = np.random.default_rng(3)
    for V in (1, 2, 37, 1025):
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        for key in range(5):
            a = R.sample_row(x, 11, key, 4, temperature=4.0, top_k=1)
            b = R.sample_row(x, 11, key, 4, temperature=0.25, top_p=1e-6)
            for r in (a, b):
                assert r["tok"] == int(np.argmax(x)) and r["nkept"] == 1 and r["logq"] == 0.0 and r["gumbel_margin"] == np.inf
            assert r["pmax"] == float(x.max()) and abs(-math.log(r["psum"]) - r["logp_model"]) < 1e-12


def test_tie_rules_on_duplicated_values():
    x = np.array([0.5, 2.0, -1.0, 2.0, 0.5, 2.0, 0.5, -np.inf], dtype=np.float32)
    # top-k cuts a run of equal values by index: the three maxima are 1, 3, 5, the tied 0.5s follow as 0, 4, 6
    for k, want in ((1, [1]), (2, [1, 3]), (3, [1, 3, 5]), (4, [1, 3, 5, 0]), (5, [1, 3, 5, 0, 4]), (6, [1, 3, 5, 0, 4, 6])):
        r = R.sample_row(x, 1, 0, 1, top_k=k)
        assert r["kept"].tolist() == want
        assert r["topk_margin"] == (0.0 if k in (1, 2, 4, 5) else 1.5)
    # -inf is never kept, whatever top_k says; with top_k >= the finite entries the filter is off
    assert R.sample_row(x, 1, 0, 1, top_k=7)["nkept"] == 7 and R.sample_row(x, 1, 0, 1)["nkept"] == 7
    # top-p cuts inside a run the same way: q = e^2 / Z each for the three maxima (0.271)
    assert R.sample_row(x, 1, 0, 1, top_p=0.5)["kept"].tolist() == [1, 3]
    assert R.sample_row(x, 1, 0, 1, top_p=0.25)["kept"].tolist() == [1]
    assert R.sample_row(x, 1, 0, 1, top_p=0.6)["kept"].tolist() == [1, 3, 5]
    # equal perturbed values cannot be constructed through the hash; equal LOGITS with one kept entry: the lowest index
    flat = np.zeros(9, dtype=np.float32)
    assert R.sample_row(flat, 5, 2, 3, top_k=1)["tok"] == 0 and R.sample_row(flat, 5, 2, 3, top_p=1e-6)["tok"] == 0
    # every draw lies in the kept set and names a maximum of s + g there
    for key in range(50):
        r = R.sample_row(x, 8, key, 2, top_k=4)
        assert r["tok"] in (1, 3, 5, 0)
    # -0.0 and +0.0 are one value: the index decides
    z = np.array([-0.0, 0.0, -0.0], dtype=np.float32)
    assert R.sample_row(z, 1, 0, 1, top_k=2)["kept"].tolist() == [0, 1]


class _FakeModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.launched = False

    def engine(self):
        self.launched = True
        raise AssertionError("a refusal must come before the engine is touched")


def test_translator_refusals_by_name():
    from care_amd.translator import Translator_ARFormer

    tr = Translator_ARFormer({"beam_size": 1, "topk": 1, "beam_alpha": 1.0, "max_len": 30})
    model = _FakeModel().eval()
    batch = {"feats": [torch.zeros(2, 28, 8)]}
    cases = [(dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("inf")), "temperature"),
             (dict(temperature=float("nan")), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"),
             (dict(top_p=float("nan")), "top_p"), (dict(top_k=-1), "top_k"), (dict(n_samples=0), "n_samples")]
    for kw, name in cases:
        with pytest.raises(ValueError, match="`{}`".format(name)):
            tr.sample_batch([model], batch, **kw)
    with pytest.raises(ValueError, match="ONE model"):
        tr.sample_batch([model, model], batch)
    with pytest.raises(ValueError, match="ONE model"):
        tr.sample_batch([], batch)
    with pytest.raises(ValueError, match="eval mode"):
        tr.sample_batch([_FakeModel().train()], batch)
    with pytest.raises(ValueError, match="CPU tensors"):
        tr.sample_batch([model], batch)
    assert not model.launched


def test_seed_none_follows_torch_manual_seed():
    from care_amd.engine_sample import draw_seed

    torch.manual_seed(1234)
    a = [draw_seed() for _ in range(3)]
    torch.manual_seed(1234)
    b = [draw_seed() for _ in range(3)]
    torch.manual_seed(1235)
    c = draw_seed()
    assert a == b and len(set(a)) == 3 and c != a[0] and all(0 <= s < 2 ** 62 for s in a + [c])


def test_abi_declares_the_sampler_in_both_libraries():
    """care_sample_logits / care_sample_accum: declared, bound, exported by both 16-bit libraries; bad arguments are refused
    on the host side of the launch (no device needed: nothing is launched)."""
    from care_amd import _lib

    for variant in ("", "f16"):
        lib = _lib.load(variant=variant)
        buf = (16 * 4) * b"\0"
        import ctypes
        mem = ctypes.create_string_buffer(buf, 64)
        p = (ctypes.addressof(mem) + 15) // 16 * 16
        ok = dict(logits=p, ld=8, V=8, rows=0, key=None, t=1, params=p, pmax=p, pidx=p, psum=p)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.care_sample_logits(a["logits"], a["ld"], a["V"], a["rows"], a["key"], a["t"], a["params"], a["pmax"], a["pidx"],
                                          a["psum"], None, None, None)
        assert call() == 0   # rows == 0: success, nothing launched
        for bad in (dict(rows=-1), dict(V=0), dict(ld=7), dict(t=0), dict(logits=None), dict(params=None), dict(pmax=None),
                    dict(pidx=None), dict(psum=None)):
            assert call(**bad) == -1, bad
        assert call(params=p + 8) == -2
        assert lib.care_sample_accum(p, p, p, 0, None) == 0 and lib.care_sample_accum(None, p, p, 1, None) == -1
        assert lib.care_sample_accum(p, p, p, -1, None) == -1
