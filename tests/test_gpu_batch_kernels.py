"""GPU: the three kernels of the device-built batch (csrc/batch.hip) alone, through the raw ABI, bit for bit against
tests/batch_reference.py.  Integers and copied bytes: nothing here has a tolerance.  Every output lies in a guarded buffer
between canaries; refused calls and empty batches must leave the whole buffer as it was.

Shapes: frame ids at (n_total, n_frames) = (60, 28) MSRVTT's, (64, 64) / (64, 1) a full wave and one frame of it, (8, 3), (1, 1);
gathered rows of 8 .. 8208 bytes - 8, 12, 24, 2046, 4092, 4104 take the 2- / 4-byte store paths, the multiples of 16 the
16-byte one, 2046 .. 8208 more than one 1-KiB piece; B = 130 rows is more than one workgroup in every kernel.

Measured on one MI355X: the 37 tests of this file 3.1 s, the slowest 0.25 s."""
import ctypes

import numpy as np
import pytest
import torch

import batch_reference as R
from care_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 64
EINVAL, EALIGN, ESHAPE, EDTYPE = -1, -2, -3, -4
CANARY = {torch.int32: -77, torch.int64: -77, torch.float32: -7.25, torch.uint8: 0xA5}
TYPES = {"equally_sampling": 0, "segment_random": 1, "all_random": 2}


def _guarded(n, dtype, shift=0):
    """(whole, view): n elements between GAP canaries on either side, on the device; shift: elements the view starts late."""
    whole = torch.full((n + 2 * GAP,), CANARY[dtype], dtype=dtype, device=DEV)
    return whole, whole[GAP + shift: GAP + shift + n]


def _untouched(whole, lo=0, hi=0):
    """Everything but whole[GAP + lo : GAP + hi] still holds the canary."""
    w = whole.cpu()
    fill = CANARY[whole.dtype]
    return bool((w[: GAP + lo] == fill).all()) and bool((w[GAP + hi:] == fill).all())


def _raw(name, *args):
    """The entry point's return code (no exception), on torch's current stream."""
    with torch.cuda.device(DEV):
        rc = getattr(_lib.load(), name)(*args, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _bounds(n_total, n_frames):
    return (ctypes.c_int32 * (n_frames + 1))(*R.snippet_bounds(n_total, n_frames))


# ------------------------------------------------------------------------------------------------------ care_batch_frame_ids
def _items(B):
    """B infoset indices that are not their place in the batch: large ones, repeats, the int32 maximum."""
    it = [(7919 * b + 13) % 200003 for b in range(B)]
    it[-1] = 2 ** 31 - 1
    if B > 2:
        it[1] = it[0]
    return it


def _frame_ids(items, n_total, n_frames, rt, seed, epoch):
    B = len(items)
    whole, out = _guarded(B * n_frames, torch.int32)
    dev_items = _dev(items)
    rc = _raw("care_batch_frame_ids", _lib.ptr(dev_items), B, n_total, n_frames, TYPES[rt], _bounds(n_total, n_frames), seed, epoch,
              _lib.ptr(out))
    assert rc == 0 and _untouched(whole, 0, B * n_frames)
    return out.cpu().numpy().reshape(B, n_frames)


@pytest.mark.parametrize("rt", sorted(TYPES))
@pytest.mark.parametrize("n_total,n_frames", [(60, 28), (64, 64), (64, 1), (8, 3), (1, 1)])
def test_frame_ids_are_the_reference_s(n_total, n_frames, rt):
    seed, epoch = 0x9E3779B97F4A7C15, 3
    for B in (1, 3, 130):
        items = _items(B)
        got = _frame_ids(items, n_total, n_frames, rt, seed, epoch)
        want = np.array([R.frame_ids(i, n_total, n_frames, rt, seed, epoch) for i in items], dtype=np.int32)
        assert np.array_equal(got, want), (B, rt)


def test_frame_ids_follow_the_item_and_the_epoch_not_the_batch():
    for rt in ("segment_random", "all_random"):
        a = _frame_ids([5, 6, 7, 8, 9], 60, 28, rt, 1, 0)
        b = _frame_ids([9, 100, 7], 60, 28, rt, 1, 0)            # items 7 and 9 in another batch, at other places
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[0])
        assert not np.array_equal(a, _frame_ids([5, 6, 7, 8, 9], 60, 28, rt, 1, 1))     # another epoch
        assert not np.array_equal(a, _frame_ids([5, 6, 7, 8, 9], 60, 28, rt, 2, 0))     # another seed
        assert len({tuple(r) for r in a}) == 5


def test_frame_ids_refusals_write_nothing():
    whole, out = _guarded(4 * 28, torch.int32)
    items = _dev([0, 1, 2, 3])
    ip, op = _lib.ptr(items), _lib.ptr(out)
    assert _raw("care_batch_frame_ids", ip, 0, 60, 28, 1, _bounds(60, 28), 0, 0, op) == 0                 # an empty batch
    assert _raw("care_batch_frame_ids", ip, 4, 60, 28, 3, _bounds(60, 28), 0, 0, op) == EDTYPE
    assert _raw("care_batch_frame_ids", ip, 4, 8, 9, 1, _bounds(8, 9), 0, 0, op) == ESHAPE                # an empty snippet
    assert _raw("care_batch_frame_ids", ip, 4, 8, 9, 2, _bounds(8, 9), 0, 0, op) == ESHAPE
    assert _raw("care_batch_frame_ids", ip, 4, 65, 28, 2, _bounds(65, 28), 0, 0, op) == ESHAPE            # all_random: one wave
    assert _raw("care_batch_frame_ids", ip, 4, 60, 129, 0, _bounds(60, 129), 0, 0, op) == ESHAPE
    assert _raw("care_batch_frame_ids", ip, 4, 60, 28, 1, _bounds(61, 28), 0, 0, op) == EINVAL            # bounds of another length
    assert _raw("care_batch_frame_ids", None, 4, 60, 28, 1, _bounds(60, 28), 0, 0, op) == EINVAL
    assert _raw("care_batch_frame_ids", ip, 4, 60, 28, 1, _bounds(60, 28), 0, 0, op + 2) == EALIGN
    assert _raw("care_batch_frame_ids", ip, -1, 60, 28, 1, _bounds(60, 28), 0, 0, op) == EINVAL
    assert _untouched(whole)
    assert _raw("care_batch_frame_ids", None, 4, 60, 28, 0, _bounds(60, 28), 0, 0, op) == 0               # equally_sampling reads no item
    assert out.cpu().view(4, 28)[3].tolist() == R.frame_ids(0, 60, 28, "equally_sampling")


# --------------------------------------------------------------------------------------------------------- care_batch_gather
N_VIDEOS, ZERO_VIDEO = 37, 5


def _table(dim, n_total, dtype, seed):
    """([n_videos, n_total, pitch / es] device table with junk in the pitch padding, its [.., dim] values as integer bit
    patterns on the host).  Video ZERO_VIDEO is all zeros (a video missing from the reference's table)."""
    es = 2 if dtype != torch.float32 else 4
    itype, nptype = (torch.int16, np.int16) if es == 2 else (torch.int32, np.int32)
    pitch = -(-dim * es // 16) * 16
    gen = torch.Generator().manual_seed(seed)
    raw = torch.randint(-2 ** 15, 2 ** 15, (N_VIDEOS, n_total, pitch // es), generator=gen, dtype=torch.int32).to(itype)
    raw[ZERO_VIDEO, :, :dim] = 0
    return raw.to(DEV), raw[:, :, :dim].numpy().astype(nptype), pitch, es


def _desc(descs, i, table, out, pitch, n_total, row_bytes, n_out):
    d = descs[i]
    d.table, d.out, d.pitch, d.n_total, d.row_bytes, d.n_out = table.data_ptr(), out.data_ptr(), pitch, n_total, row_bytes, n_out


def _ids(B, n_total, n_frames, seed):
    rng = np.random.RandomState(seed)
    vids = rng.randint(0, N_VIDEOS, size=B).astype(np.int32)
    vids[0] = ZERO_VIDEO
    if B > 2:
        vids[2] = vids[1]                                            # a video twice in a batch
    fids = rng.randint(0, n_total, size=(B, n_frames)).astype(np.int32)   # any order, repeats: a gather, not a slice
    return vids, fids


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "h16"])
@pytest.mark.parametrize("dim", [4, 6, 512, 1023, 2052])
def test_gather_copies_the_rows(dim, dtype):
    for n_total in (1, 8, 60):
        table, host, pitch, es = _table(dim, n_total, dtype, 100 + n_total)
        row_bytes = dim * es
        for n_frames in (1, 8, 28):
            for B in (1, 3, 130):
                vids, fids = _ids(B, n_total, n_frames, B + n_frames)
                n = B * n_frames * row_bytes
                whole, out = _guarded(n, torch.uint8)
                descs = (_lib.BatchTable * 1)()
                _desc(descs, 0, table, out, pitch, n_total, row_bytes, n_frames)
                dv, df = _dev(vids), _dev(fids)
                rc = _raw("care_batch_gather", descs, 1, _lib.ptr(dv), _lib.ptr(df), N_VIDEOS, B, n_frames)
                assert rc == 0 and _untouched(whole, 0, n), (n_total, n_frames, B)
                want = host[vids[:, None], np.zeros_like(fids) if n_total == 1 else fids]
                got = out.cpu().numpy().view(host.dtype).reshape(B, n_frames, dim)
                assert np.array_equal(got, want), (n_total, n_frames, B)
                assert not got[0].any()


def test_gather_three_modalities_one_launch_and_ids_outside_the_tables():
    """m: 60 frames x 2048 B, i: a per-video vector of 24 B (the launch's store unit becomes 4 bytes), r: one block of
    5 x 64 B a video; items with a video id of -1 and of n_videos and a frame id of n_total and of -1 are zero rows."""
    B, n_frames = 130, 28
    tm, hm, pm, _ = _table(512, 60, torch.float32, 1)
    ti, hi, pi, _ = _table(6, 1, torch.float32, 2)
    tr, hr, pr, _ = _table(5 * 16, 1, torch.float32, 3)
    vids, fids = _ids(B, 60, n_frames, 9)
    vids[7], vids[8], vids[9], fids[9, 3], fids[10, 0] = -1, N_VIDEOS, 11, 60, -1
    sizes = [B * n_frames * 2048, B * n_frames * 24, B * 320]
    bufs = [_guarded(s, torch.uint8) for s in sizes]
    descs = (_lib.BatchTable * 3)()
    _desc(descs, 0, tm, bufs[0][1], pm, 60, 2048, n_frames)
    _desc(descs, 1, ti, bufs[1][1], pi, 1, 24, n_frames)
    _desc(descs, 2, tr, bufs[2][1], pr, 1, 320, 1)
    dv, df = _dev(vids), _dev(fids)
    assert _raw("care_batch_gather", descs, 3, _lib.ptr(dv), _lib.ptr(df), N_VIDEOS, B, n_frames) == 0
    ok_v = (vids >= 0) & (vids < N_VIDEOS)
    v = np.where(ok_v, vids, 0)
    ok_f = (fids >= 0) & (fids < 60)
    want_m = hm[v[:, None], np.where(ok_f, fids, 0)] * (ok_v[:, None] & ok_f)[:, :, None]
    want_i = np.repeat(hi[v][:, :1], n_frames, axis=1) * ok_v[:, None, None]
    want_r = hr[v][:, 0] * ok_v[:, None]
    for (whole, out), want, size in zip(bufs, (want_m, want_i, want_r), sizes):
        assert _untouched(whole, 0, size)
        assert np.array_equal(out.cpu().numpy().view(np.int32).reshape(want.shape), want)
    assert not want_m[7].any() and not want_m[9, 3].any() and want_m[9, 2].any()


@pytest.mark.parametrize("shift", [2, 4, 8])
def test_gather_into_an_output_that_is_not_16_byte_aligned(shift):
    """Rows of 2048 bytes into an output `shift` bytes off a 16-byte boundary: the 2- and 4-byte store paths with whole rows."""
    B, n_frames = 3, 8
    table, host, pitch, es = _table(1024, 8, torch.bfloat16, 4)
    vids, fids = _ids(B, 8, n_frames, 5)
    n = B * n_frames * 2048
    whole, out = _guarded(n + 16, torch.uint8, shift)
    out = out[:n]
    descs = (_lib.BatchTable * 1)()
    _desc(descs, 0, table, out, pitch, 8, 2048, n_frames)
    assert out.data_ptr() % 16 == shift
    dv, df = _dev(vids), _dev(fids)
    assert _raw("care_batch_gather", descs, 1, _lib.ptr(dv), _lib.ptr(df), N_VIDEOS, B, n_frames) == 0
    assert _untouched(whole, shift, shift + n)
    assert np.array_equal(out.cpu().numpy().view(np.int16).reshape(B, n_frames, 1024), host[vids[:, None], fids])


def test_gather_refusals_write_nothing():
    table, _, pitch, _ = _table(6, 8, torch.float32, 6)
    whole, out = _guarded(4 * 3 * 24, torch.uint8)
    vids, fids = _dev([0, 1, 2, 3]), _dev(np.zeros((4, 3)))
    vp, fp = _lib.ptr(vids), _lib.ptr(fids)

    def call(count=1, B=4, n_videos=N_VIDEOS, n_frames=3, v=vp, f=fp, **over):
        descs = (_lib.BatchTable * 9)()
        for i in range(9):
            _desc(descs, i, table, out, pitch, 8, 24, 3)
            for k, val in over.items():
                setattr(descs[i], k, val)
        return _raw("care_batch_gather", descs, count, v, f, n_videos, B, n_frames)

    assert call(B=0) == 0                                       # an empty batch
    assert call(count=0) == EINVAL and call(count=9) == ESHAPE
    assert call(B=-1) == EINVAL and call(n_videos=0) == EINVAL and call(v=None) == EINVAL and call(f=None) == EINVAL
    assert call(table=None) == EINVAL and call(out=None) == EINVAL
    assert call(row_bytes=23) == EINVAL and call(row_bytes=0) == EINVAL and call(pitch=16) == EINVAL and call(n_total=0) == EINVAL
    assert call(n_out=2) == ESHAPE                              # frames of a table with n_total > 1: n_out == n_frames
    assert call(pitch=40) == EALIGN and call(table=table.data_ptr() + 8) == EALIGN and call(out=out.data_ptr() + 1) == EALIGN
    assert call(v=vp + 2) == EALIGN
    assert _untouched(whole)


# ----------------------------------------------------------------------------------------------------------- care_batch_text
MAX_LEN = 8
A0, A_END = R.ATTRIBUTE_START, R.ATTRIBUTE_END


def _corpus():
    """Two videos: `one` with a single caption, `many` with 20 - lengths 2, 7, 8, 9, 15 against max_len 8, and the tokens at
    either end of every attribute range under test (n_attributes 1, 33, 3000)."""
    B_, E_ = R.BOS, R.EOS
    edge = [A0 - 1, A0, A0 + 1, A0 + 31, A0 + 32, A0 + 33, A_END - 1, A_END, 1]
    many = [[B_, E_],                                                   # 2
            [B_, 4100, 4101, 4102, 4103, 4104, E_],                     # 7 (words from 4000 on are no attributes)
            [B_, 4200, 4201, 4202, 4203, 4204, 4205, E_],               # 8 = max_len
            [B_, 4300, 4301, 4302, 4303, 4304, 4305, 4306, E_],         # 9: cut, EOS forced
            [B_] + list(range(4400, 4413)) + [E_]]                      # 15
    many += [[B_, edge[k % len(edge)], 5000 + k, E_] for k in range(14)]
    many.append([B_, 6000, E_])
    assert len(many) == 20
    one = [[B_, A0 + 2, A_END - 2, E_]]
    return {"one": one, "many": many, "ends": [[B_, A0 + 5, E_], [B_, A0 + 40, A0 + 2998, E_]]}, ["one", "many", "ends"]


def _caption_table(captions, names):
    tokens, cap_start, cap_video, vid_first = [], [0], [], [0]
    for v, name in enumerate(names):
        for cap in captions[name]:
            tokens += cap
            cap_start.append(len(tokens))
            cap_video.append(v)
        vid_first.append(len(cap_video))
    return [_dev(a) for a in (tokens, cap_start, cap_video, vid_first)], len(cap_video)


@pytest.mark.parametrize("n_attr", [1, 33, 3000])
def test_text_is_the_reference_s(n_attr):
    captions, names = _corpus()
    (tokens, cap_start, cap_video, vid_first), n_caps = _caption_table(captions, names)
    flat = [(v, c) for v, name in enumerate(names) for c in range(len(captions[name]))]
    item_cap = _dev(np.arange(n_caps)[::-1].copy())                     # item i is caption n_caps - 1 - i
    for B in (1, 3, 130):
        items = [(5 * b + 1) % n_caps for b in range(B)]
        W = MAX_LEN - 1
        wv, vid = _guarded(B, torch.int32)
        wc, cid = _guarded(B, torch.int32)
        wi, inp = _guarded(B * W, torch.int64)
        wl, lab = _guarded(B * W, torch.int64)
        wa, att = _guarded(B * n_attr, torch.float32)
        dev_items = _dev(items)
        rc = _raw("care_batch_text", _lib.ptr(dev_items), B, _lib.ptr(item_cap), n_caps, _lib.ptr(tokens), _lib.ptr(cap_start),
                  _lib.ptr(cap_video), _lib.ptr(vid_first), n_caps, len(names), MAX_LEN, R.PAD, R.EOS, A0, n_attr, _lib.ptr(vid),
                  _lib.ptr(cid), _lib.ptr(inp), _lib.ptr(lab), _lib.ptr(att))
        assert rc == 0
        for whole, n in ((wv, B), (wc, B), (wi, B * W), (wl, B * W), (wa, B * n_attr)):
            assert _untouched(whole, 0, n)
        pairs = [flat[n_caps - 1 - i] for i in items]
        assert vid.cpu().tolist() == [v for v, _ in pairs] and cid.cpu().tolist() == [c for _, c in pairs]
        st = [R.source_target(captions[names[v]][c], MAX_LEN) for v, c in pairs]
        assert inp.cpu().view(B, W).tolist() == [s for s, _ in st]
        assert lab.cpu().view(B, W).tolist() == [t for _, t in st]
        want = np.stack([R.attribute_labels(captions[names[v]], n_attr) for v, _ in pairs])
        assert np.array_equal(att.cpu().numpy().reshape(B, n_attr), want)
    if n_attr == 3000:   # the boundary tokens did what they should
        lab_many = R.attribute_labels(captions["many"], 3000)
        assert np.flatnonzero(lab_many).tolist() == [0, 1, 31, 32, 33, 2999]


def test_text_without_concept_labels_and_items_outside_the_infoset():
    captions, names = _corpus()
    (tokens, cap_start, cap_video, vid_first), n_caps = _caption_table(captions, names)
    item_cap = _dev(np.arange(n_caps))
    items, B, W = [3, -1, n_caps, 0], 4, MAX_LEN - 1
    wv, vid = _guarded(B, torch.int32)
    wc, cid = _guarded(B, torch.int32)
    wi, inp = _guarded(B * W, torch.int64)
    wl, lab = _guarded(B * W, torch.int64)
    dev_items = _dev(items)
    rc = _raw("care_batch_text", _lib.ptr(dev_items), B, _lib.ptr(item_cap), n_caps, _lib.ptr(tokens), _lib.ptr(cap_start),
              _lib.ptr(cap_video), _lib.ptr(vid_first), n_caps, len(names), MAX_LEN, R.PAD, R.EOS, A0, 0, _lib.ptr(vid),
              _lib.ptr(cid), _lib.ptr(inp), _lib.ptr(lab), None)
    assert rc == 0 and all(_untouched(w, 0, n) for w, n in ((wv, B), (wc, B), (wi, B * W), (wl, B * W)))
    assert vid.cpu().tolist() == [1, -1, -1, 0] and cid.cpu().tolist() == [2, -1, -1, 0]
    assert inp.cpu().view(B, W)[1].tolist() == [R.PAD] * W and lab.cpu().view(B, W)[2].tolist() == [R.PAD] * W
    assert inp.cpu().view(B, W)[0].tolist() == R.source_target(captions["many"][2], MAX_LEN)[0]


def test_text_refusals_write_nothing():
    captions, names = _corpus()
    (tokens, cap_start, cap_video, vid_first), n_caps = _caption_table(captions, names)
    item_cap, items = _dev(np.arange(n_caps)), _dev([0, 1])
    W = MAX_LEN - 1
    bufs = [_guarded(2, torch.int32), _guarded(2, torch.int32), _guarded(2 * W, torch.int64), _guarded(2 * W, torch.int64),
            _guarded(2 * 33, torch.float32)]
    outs = [_lib.ptr(v) for _, v in bufs]

    def call(B=2, n_items=n_caps, max_len=MAX_LEN, n_attr=33, it=_lib.ptr(items), o=outs):
        return _raw("care_batch_text", it, B, _lib.ptr(item_cap), n_items, _lib.ptr(tokens), _lib.ptr(cap_start), _lib.ptr(cap_video),
                    _lib.ptr(vid_first), n_caps, len(names), max_len, R.PAD, R.EOS, A0, n_attr, *o)

    assert call(B=0) == 0
    assert call(B=-1) == EINVAL and call(n_items=0) == EINVAL and call(max_len=1) == EINVAL and call(it=None) == EINVAL
    assert call(o=outs[:2] + [None] + outs[3:]) == EINVAL
    assert call(n_attr=0) == ESHAPE and call(n_attr=3001) == ESHAPE
    assert call(o=outs[:2] + [outs[2] + 4] + outs[3:]) == EALIGN and call(o=[outs[0] + 2] + outs[1:]) == EALIGN
    assert all(_untouched(w) for w, _ in bufs)
