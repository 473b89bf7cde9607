"""GPU: the kernels of the mean-teacher step (csrc/interplay.hip) through the raw ABI - care_ema_step against the BITS of torch's
three `_foreach` calls, care_mse_fwd / care_mse_bwd against float64 within the bar derived in tests/interplay_reference.py.

The sizes are those at which vector bodies, scalar tails, chunk boundaries, launch splitting and the peel to the 16-byte boundary
can go wrong: 1, 3, 4, 5 elements, one chunk of 1024 and its neighbours, several workgroups in one tensor, a list longer than two
launches, the logits of two captions of seven positions (V = 10547 is odd) and an array that gives every workgroup of the full
grid more than one chunk; every one of them with 16-byte aligned bases, with bases one element behind, and mixed."""
import functools
import math
import os
import re

import pytest
import torch

import interplay_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 8              # canary floats between and around the tensors
CANARY = -7.25
EINVAL, EALIGN = -1, -2
EMA_SIZES = (1, 3, 4, 5, 1023, 0, 1024, 1025, 4099, 52736)    # 52736 = 51 chunks + a tail; one empty tensor in the middle
T_SHIFTED, S_SHIFTED = (3, 7), (4, 8)                         # tensors that start one element past a 16-byte boundary, by side
V = 10547
MSE_BIG = 2 * 2048 * 1024 + 1027                               # 4097 chunks for 2048 workgroups: two or three each
MSE_SIZES = (1, 3, 4, 1023, 1024, 1025, 2 * 7 * V, MSE_BIG)
PHASES = ((0, 0), (1, 1), (0, 1))                              # (a, b): elements past the 16-byte boundary


def _ema_pack():
    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    return int(re.search(r"#define CARE_EMA_PACK (\d+)", header).group(1))


def _offsets(sizes, shifted):
    out, pos = [], GAP
    for i, n in enumerate(sizes):
        start = (pos + 3) // 4 * 4 + (1 if i in shifted else 0)
        out.append(start)
        pos = start + n + GAP
    return out, pos


def _flat(values, offsets, total):
    flat = torch.full((total,), CANARY, dtype=torch.float32)
    for v, o in zip(values, offsets):
        flat[o:o + v.numel()] = v
    return flat


def _ema_case(sizes, t_shifted, s_shifted, seed):
    """Two flat buffers (teacher, student) with the tensors of `sizes` at their offsets and canaries everywhere else."""
    g = torch.Generator().manual_seed(seed)
    scales = [10.0 ** (-3 + 6 * i / max(1, len(sizes) - 1)) for i in range(len(sizes))]      # 1e-3 .. 1e3 by tensor
    t = [torch.randn(n, generator=g) * sc for n, sc in zip(sizes, scales)]
    s = [torch.randn(n, generator=g) * sc for n, sc in zip(sizes, scales)]
    off_t, total_t = _offsets(sizes, t_shifted)
    off_s, total_s = _offsets(sizes, s_shifted)
    return t, s, off_t, off_s, _flat(t, off_t, total_t), _flat(s, off_s, total_s)


def _ema_descs(flat_t, flat_s, off_t, off_s, sizes):
    from care_amd import _lib

    assert flat_t.data_ptr() % 16 == 0 and flat_s.data_ptr() % 16 == 0
    d = (_lib.EmaTensor * len(sizes))()
    for i, n in enumerate(sizes):
        d[i].t, d[i].s, d[i].n = flat_t.data_ptr() + 4 * off_t[i], flat_s.data_ptr() + 4 * off_s[i], n
    return d


def _run_ema(sizes, t_shifted, s_shifted, w, seed):
    from care_amd import _lib

    t, s, off_t, off_s, flat_t, flat_s = _ema_case(sizes, t_shifted, s_shifted, seed)
    dev_t, dev_s = flat_t.to(DEV), flat_s.to(DEV)
    d = _ema_descs(dev_t, dev_s, off_t, off_s, sizes)
    _lib.call("care_ema_step", d, len(sizes), w, 1 - w)
    torch.cuda.synchronize()
    want = _flat(R.ema_reference(t, s, w), off_t, flat_t.numel())       # the reference's tensors between untouched canaries
    return R.bits(dev_t), R.bits(want), R.bits(dev_s), R.bits(flat_s), (t, s, off_t, dev_t)


@pytest.mark.parametrize("w", [0.999, 0.5])
def test_ema_step_has_the_bits_of_the_three_foreach_calls(w):
    for i in T_SHIFTED + S_SHIFTED:
        assert EMA_SIZES[i] > 4
    got, want, student, student_before, _ = _run_ema(EMA_SIZES, T_SHIFTED, S_SHIFTED, w, seed=21)
    bad = (got != want).nonzero().reshape(-1)
    assert bad.numel() == 0, "teacher bits or canaries differ at flat offsets {} ...".format(bad[:8].tolist())
    assert torch.equal(student, student_before), "s is read, never written"


def test_ema_step_over_more_tensors_than_two_launches_hold():
    pack = _ema_pack()
    sizes = tuple(1 + i % 40 for i in range(2 * pack + 2))
    assert math.ceil(len(sizes) / pack) == 3
    got, want, student, student_before, _ = _run_ema(sizes, (3, pack, 2 * pack + 1), (5, pack + 1), 0.999, seed=22)
    assert torch.equal(got, want) and torch.equal(student, student_before)


def test_ema_step_identities():
    """w = 1 keeps the teacher's bits; w = 0 gives the student's VALUES (a student of -0 against a teacher >= 0 gives +0)."""
    got, _, _, _, (t, s, off_t, _) = _run_ema(EMA_SIZES, T_SHIFTED, S_SHIFTED, 1.0, seed=23)
    assert torch.equal(got, R.bits(_flat(t, off_t, got.numel())))
    _, _, _, _, (t, s, off_t, dev_t) = _run_ema(EMA_SIZES, T_SHIFTED, S_SHIFTED, 0.0, seed=24)
    assert torch.equal(dev_t.cpu(), _flat(s, off_t, dev_t.numel()))


def test_ema_step_edge_cases_and_refusals():
    from care_amd import _lib

    lib = _lib.load()
    t, s, off_t, off_s, flat_t, flat_s = _ema_case(EMA_SIZES, T_SHIFTED, S_SHIFTED, seed=25)
    dev_t, dev_s = flat_t.to(DEV), flat_s.to(DEV)
    d = _ema_descs(dev_t, dev_s, off_t, off_s, EMA_SIZES)
    n = len(EMA_SIZES)
    stream = _lib.stream_ptr()
    assert lib.care_ema_step(d, 0, 0.5, 0.5, stream) == 0 and lib.care_ema_step(None, 0, 0.5, 0.5, stream) == 0
    assert lib.care_ema_step(None, n, 0.5, 0.5, stream) == EINVAL
    keep = d[3].t
    d[3].t = None
    assert lib.care_ema_step(d, n, 0.5, 0.5, stream) == EINVAL
    d[3].t = d[3].s
    assert lib.care_ema_step(d, n, 0.5, 0.5, stream) == EINVAL          # a tensor paired with itself
    d[3].t = keep + 2
    assert lib.care_ema_step(d, n, 0.5, 0.5, stream) == EALIGN
    d[3].t = keep
    keep = d[9].s
    d[9].s = keep + 2
    assert lib.care_ema_step(d, n, 0.5, 0.5, stream) == EALIGN
    d[9].s = keep
    d[1].n = -1
    assert lib.care_ema_step(d, n, 0.5, 0.5, stream) == EINVAL
    d[1].n = EMA_SIZES[1]
    torch.cuda.synchronize()
    assert torch.equal(R.bits(dev_t), R.bits(flat_t)) and torch.equal(R.bits(dev_s), R.bits(flat_s)), "a refused call writes nothing"
    # ... and the descriptors were left valid: the same list now runs
    _lib.call("care_ema_step", d, n, 0.5, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(dev_t), R.bits(_flat(R.ema_reference(t, s, 0.5), off_t, flat_t.numel())))


# ------------------------------------------------------------------ the distillation term
def _place(values, phase):
    """A device buffer of GAP canaries | `phase` more | values | GAP canaries; returns (whole, view)."""
    off = GAP + phase
    whole = torch.full((off + values.numel() + GAP,), CANARY, dtype=torch.float32)
    whole[off:off + values.numel()] = values
    whole = whole.to(DEV)
    view = whole[off:off + values.numel()]
    assert view.data_ptr() % 16 == 4 * phase
    return whole, view


def _canaries_intact(whole, n, phase):
    w = whole.cpu()
    return bool((w[:GAP + phase] == CANARY).all()) and bool((w[GAP + phase + n:] == CANARY).all())


@functools.lru_cache(maxsize=None)
def _mse_data(n, kind):
    """(a, b, float64 loss, float64 gradient for g = fp32(0.01)); every seventh element of b equals a's."""
    g = torch.Generator().manual_seed(1000 + n % 997)
    if kind == "plain":
        a = torch.randn(n, generator=g)
        b = a + 0.05 * torch.randn(n, generator=g)
    else:            # cancellation: values around 5e3 whose differences are around 1e-3
        a = 5e3 + torch.randn(n, generator=g)
        b = a + 1e-3 * torch.randn(n, generator=g)
    if n >= 7:
        b[::7] = a[::7]
    return a, b, R.mse_reference64(a, b), R.mse_grad_reference64(a, b, float(torch.tensor(0.01, dtype=torch.float32)))


def _mse_fwd(a, b):
    from care_amd import _lib

    n = a.numel()
    partials = torch.full((_lib.load().care_mse_partials(n),), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    _lib.call("care_mse_fwd", a.data_ptr(), b.data_ptr(), n, partials.data_ptr(), loss.data_ptr())
    return loss


@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_fwd_against_float64(n):
    from care_amd import _lib

    assert _lib.load().care_mse_partials(MSE_BIG) == 2048 and MSE_BIG // 1024 >= 2 * 2048
    kinds = ("plain", "cancel") if n in (1025, 2 * 7 * V) else ("plain",)
    for kind in kinds:
        a, b, want, _ = _mse_data(n, kind)
        for pa, pb in PHASES:
            (wa, va), (wb, vb) = _place(a, pa), _place(b, pb)
            one, two = _mse_fwd(va, vb), _mse_fwd(va, vb)
            got = float(one)
            print("n", n, kind, "phases", pa, pb, "loss", got, "float64", want, "relative deviation",
                  abs(got - want) / want if want else 0.0, "bar", R.BAR)
            assert abs(got - want) <= R.BAR * want, (n, kind, pa, pb, got, want)
            assert torch.equal(R.bits(one), R.bits(two)), "two calls must give the same bits"
            assert torch.equal(R.bits(va), R.bits(a)) and torch.equal(R.bits(vb), R.bits(b)), "the operands are read, never written"
            assert _canaries_intact(wa, n, pa) and _canaries_intact(wb, n, pb)
            assert float(_mse_fwd(va, va.clone())) == 0.0, "a == b gives exactly 0"


def test_mse_fwd_non_finite_input_and_refusals():
    from care_amd import _lib

    lib = _lib.load()
    a, b, _, _ = _mse_data(1025, "plain")
    a = a.clone()
    a[700] = float("inf")
    (_, va), (_, vb) = _place(a, 1), _place(b, 1)
    assert not math.isfinite(float(_mse_fwd(va, vb))), "an inf in the logits is not hidden"
    partials = torch.zeros(4, dtype=torch.float64, device=DEV)
    loss = torch.zeros(2, device=DEV)
    A, B, P, L, stream = va.data_ptr(), vb.data_ptr(), partials.data_ptr(), loss.data_ptr(), _lib.stream_ptr()
    assert lib.care_mse_fwd(None, B, 1025, P, L, stream) == EINVAL and lib.care_mse_fwd(A, None, 1025, P, L, stream) == EINVAL
    assert lib.care_mse_fwd(A, B, 1025, None, L, stream) == EINVAL and lib.care_mse_fwd(A, B, 1025, P, None, stream) == EINVAL
    assert lib.care_mse_fwd(A, B, 0, P, L, stream) == EINVAL
    assert lib.care_mse_fwd(A, B, 1025, P + 4, L, stream) == EALIGN, "partials at an odd 4-byte address"
    assert lib.care_mse_fwd(A + 2, B, 1025, P, L, stream) == EALIGN
    g = torch.zeros(1, device=DEV)
    da = torch.full((1025 + 8,), CANARY, device=DEV)
    G, D = g.data_ptr(), da.data_ptr()
    assert lib.care_mse_bwd(None, B, 1025, G, D, stream) == EINVAL and lib.care_mse_bwd(A, B, 1025, None, D, stream) == EINVAL
    assert lib.care_mse_bwd(A, B, 1025, G, None, stream) == EINVAL and lib.care_mse_bwd(A, B, 0, G, D, stream) == EINVAL
    assert lib.care_mse_bwd(A, B, 1025, G, D + 2, stream) == EALIGN and lib.care_mse_bwd(A, B + 1, 1025, G, D, stream) == EALIGN
    torch.cuda.synchronize()
    assert bool((partials == 0).all()) and bool((loss == 0).all()) and bool((da == CANARY).all()), "a refused call writes nothing"


@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_bwd_against_float64(n):
    from care_amd import _lib

    g = torch.tensor([0.01], dtype=torch.float32, device=DEV)
    zero = torch.zeros(1, dtype=torch.float32, device=DEV)
    kinds = ("plain", "cancel") if n in (1025, 2 * 7 * V) else ("plain",)
    for kind in kinds:
        a, b, _, want = _mse_data(n, kind)
        equal = a == b
        assert bool((want[equal] == 0).all()) and bool((want[~equal] != 0).all())
        for pa, pb, pd in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 1, 0)):
            (_, va), (_, vb) = _place(a, pa), _place(b, pb)
            whole, da = _place(torch.full((n,), float("nan")), pd)
            _lib.call("care_mse_bwd", va.data_ptr(), vb.data_ptr(), n, g.data_ptr(), da.data_ptr())
            got = da.cpu().double()
            assert bool((got[equal] == 0).all()), "the gradient is exactly 0 where a_i == b_i"
            dev = ((got - want).abs()[~equal] / want.abs()[~equal]).max().item() if bool((~equal).any()) else 0.0
            print("n", n, kind, "phases", pa, pb, pd, "worst relative deviation", dev, "bar", R.BAR)
            assert dev <= R.BAR, (n, kind, pa, pb, pd, dev)
            assert _canaries_intact(whole, n, pd), (n, pa, pb, pd)
            assert torch.equal(R.bits(va), R.bits(a)) and torch.equal(R.bits(vb), R.bits(b))
            _lib.call("care_mse_bwd", va.data_ptr(), vb.data_ptr(), n, zero.data_ptr(), da.data_ptr())
            assert bool((da == 0).all()), "g = 0 gives all zeros"
            assert _canaries_intact(whole, n, pd)
