"""LOOKUP COUNTS on the device (hrx_lookup_counts_device / _planes, lookup_counts_kernel of csrc/hrx_kernel_lookup.hip).  The rows come from the device witness
entry points; the yardsticks are the host twin (hrx_lookup_counts_host over the same rows copied to the host), word for word, and tests/lookup_ref.py on a
sample of strings — neither is the kernel under test.

  forms and shapes     sm, sm-pitched, pm, pm-in, planes (one def: the two row stripes) x batches around the group size the planner reports x 1, 5, 19, 1024 rows
  windows              across the position-major block border; starting and ending inside a group
  defs                 five and eight
  bin-range passes     the synthetic 256-state DFA: 65537 transition rows, two passes
  contention           empty strings (every row hits row 0); one repeated byte with one bin beyond 65535
  tamper               the tamper matrix of test_verify_gpu.py on the device copy: misses where the device verdict has a lookup bit
  contract             first call inside a capture, capture and replay, a side stream, refused calls, a host-only context

Every counts and misses buffer lies between two poisoned 4-KiB guards."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fr_cases as fc
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from lookup_ref import LookupRef
from oracle_lib import OracleDefs
from test_match_cpu import CFG_H4, CFG_23
from test_verify_gpu import Rows, defs_of_files, defs_of_text, tamper_batch, CFG_1, CFG_A, CFG_123, PM, PM_IN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POISON = 0x5A5A5A5A
GUARD = 1024                  # u32 words: 4 KiB before and behind
LOOKUP_BITS = hra.VERIFY_TRANSITION | hra.VERIFY_START_LOOKUP | hra.VERIFY_END_LOOKUP
FORMS = ("sm", "sm-pitched", "pm", "pm-in", "planes")


def guarded(n):
    raw = torch.full((GUARD + n + GUARD,), POISON, dtype=torch.int32, device=DEV)
    return raw, raw[GUARD:GUARD + n]


def intact(raw, n):
    return bool((raw[:GUARD] == POISON).all()) and bool((raw[GUARD + n:] == POISON).all())


def device_counts(rows, b_begin=0, b_count=None, stream=None, cfg=None):
    """the device counts and misses of a window between their guards, as uint32"""
    cfg = cfg or rows.cfg
    b_count = rows.B - b_begin if b_count is None else b_count
    W = cfg.lookup_words()
    raw, flat = guarded(b_count * W)
    rawm, mo = guarded(b_count)
    out, m = cfg.lookup_counts(rows.src, rows.d_lens, rows.rec, layout=rows.layout, planes=rows.planes, b_begin=b_begin, b_count=b_count, out=flat.view(b_count, W),
                               misses=mo, stream=stream, **rows.kw)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert out.data_ptr() == flat.data_ptr() and intact(raw, b_count * W) and intact(rawm, b_count), rows.form + ": a guard was written"
    return flat.view(b_count, W).cpu().numpy().view(np.uint32), mo.cpu().numpy().view(np.uint32)


def host_counts(rows, b_begin=0, b_count=None):
    rec, msk = rows.host_rows()
    return rows.cfg.lookup_counts_host(rows.chars, rows.lens, rec, b_begin=b_begin, b_count=b_count)


def same_as_host(rows, b_begin=0, b_count=None):
    got, gm = device_counts(rows, b_begin, b_count)
    want, wm = host_counts(rows, b_begin, b_count)
    bad = np.nonzero((got != want).any(1) | (gm != wm))[0]
    assert not len(bad), "%s B=%d M=%d window %d+%s: string %d differs from the host twin" % (rows.form, rows.B, rows.M, b_begin, b_count, b_begin + bad[0])
    lay = rows.cfg.lookup_layout()
    assert not got[:, lay[-1]["end"].stop:].any()              # the pad words
    return got, gm


def against_ref(rows, ref, got, gm, sample, b_begin=0):
    rec, msk = rows.host_rows()
    for b in sample:
        run, miss = ref.count_records(rows.chars[b], int(rows.lens[b]), rows.M, rec[b])
        assert np.array_equal(got[b - b_begin], run) and int(gm[b - b_begin]) == miss.sum(), (rows.form, b)


def batch(B, M, seed=3):
    chars, lens = synth.ragged(B, M, seed=seed)
    lens = np.minimum(lens, M).astype(np.uint32)
    if B > 2:
        lens[0], lens[1] = 0, M
    return np.ascontiguousarray(chars), lens


def largest_group_from(cfg, G):
    """the smallest batch for which the planner keeps the largest group G (below it two workgroups per CU come first)"""
    lo, hi = 1, 1 << 20
    while lo < hi:
        mid = (lo + hi) // 2
        if cfg.lookup_group(mid)[0] == G:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("M", [1, 5, 19, 1024])
def test_every_form_around_the_group_size(oracle, M):
    """regex1 + regex2.  B = 1, 65, 300: the planner lowers the group to one string (two workgroups per CU come first); with Bt the smallest batch that gets
    the largest group G the bins allow: Bt - 1 (the group is halved), Bt (the last group holds one string), Bt + 1, Bt + G - 1 (every group is full)"""
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    ref = LookupRef(OracleDefs.from_files(oracle, CFG_A))
    G = cfg.lookup_group(1 << 20)[0]
    Bt = largest_group_from(cfg, G)
    assert G >= 2 and cfg.lookup_group(Bt) == (G, 1) and cfg.lookup_group(Bt - 1) == (G // 2, 1) and cfg.lookup_group(300) == (1, 1) and Bt % G == 1
    sizes = [1, 65, 300] + ([Bt - 1, Bt, Bt + 1, Bt + G - 1] if M < 1024 else [])
    for B in sizes:
        chars, lens = batch(B, M, seed=B)
        for form in FORMS:
            rows = Rows(cfg, form, chars, lens)
            got, gm = same_as_host(rows)
            if form in ("sm", "pm-in"):
                against_ref(rows, ref, got, gm, sorted({0, B // 2, B - 1}))
    if M == 1024:
        chars, lens = batch(Bt + G, M, seed=9)
        same_as_host(Rows(cfg, "pm-in", chars, lens))
        same_as_host(Rows(cfg, "sm", chars, lens), 0, Bt)


@pytest.mark.parametrize("form", ["pm", "pm-in"])
def test_windows(oracle, form):
    """65536 + 300 strings x 19 rows of sweep_def(40): a window across the position-major block border (the second block's string count enters every index), a
    window that starts and ends inside a group of the whole batch's cut, a window of one string, the batch's last strings"""
    chars, lens = fc.tall_batch()
    B, M = len(lens), 19
    defs_t = [fc.sweep_def(fc.BIG_SWEEP_L)]
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(defs_t), device=0)
    rows = Rows(cfg, form, chars, lens)
    ref = LookupRef(OracleDefs(oracle, [(defs_t[0][0].encode(), [s.encode() for s in defs_t[0][1]])]))
    got, gm = same_as_host(rows, 65528, 24)
    against_ref(rows, ref, got, gm, [65528, 65535, 65536, 65551], b_begin=65528)
    G = cfg.lookup_group(B)[0]
    n = largest_group_from(cfg, G) + G + 4
    assert G >= 4 and cfg.lookup_group(n)[0] == G and n % G and n + 3 < 65536
    got, gm = same_as_host(rows, 3, n)
    against_ref(rows, ref, got, gm, [3, n + 2], b_begin=3)
    same_as_host(rows, 65535, 1)
    same_as_host(rows, B - 7, 7)


@pytest.mark.parametrize("name,names", [("five", CFG_H4 + CFG_23[:1]), ("eight", CFG_H4 * 2)])
def test_five_and_eight_defs(oracle, name, names):
    M = 64
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0)
    ref = LookupRef(OracleDefs.from_files(oracle, names))
    G = cfg.lookup_group(1 << 20)[0]
    for B in (300, largest_group_from(cfg, G) + 2):
        chars, lens = batch(B, M, seed=B)
        for form in ("sm", "pm-in", "planes"):
            rows = Rows(cfg, form, chars, lens)
            got, gm = same_as_host(rows)
            if form == "pm-in":
                against_ref(rows, ref, got, gm, [0, 1, B - 1])


def test_bin_range_passes(oracle):
    """the synthetic 256-state DFA: 65537 transition rows, 258 KiB of bins per string: two passes over the rows at one string per workgroup"""
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    M, B = 4096, 3
    cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=0)
    assert cfg.lookup_group(B) == (1, 2)
    chars, lens = synth.noise(B, M, seed=1, alphabet=np.arange(256, dtype=np.uint8))
    lens[1] = 1000
    ref = LookupRef(OracleDefs(oracle, [(a_txt.encode() if isinstance(a_txt, str) else a_txt, [sub_txt.encode() if isinstance(sub_txt, str) else sub_txt])]))
    for form in ("pm-in", "sm", "planes"):
        rows = Rows(cfg, form, np.ascontiguousarray(chars), lens)
        got, gm = same_as_host(rows)
        assert not gm.any() and (got[:, :65537].sum(1) == [M - 1, M, M - 1]).all()
        if form == "pm-in":
            against_ref(rows, ref, got, gm, [1])
    same_as_host(rows, 1, 2)


def test_contention_and_wide_counts():
    """every add of a string on one LDS word.  Empty strings: every row's three tuples are the dummy rows.  One repeated byte, 65600 rows: one bin beyond 65535"""
    M, B = 1024, 300
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    lay = cfg.lookup_layout()[0]
    chars, lens = batch(B, M)
    rows = Rows(cfg, "pm-in", chars, np.zeros(B, np.uint32))
    got, gm = same_as_host(rows)
    assert (got[:, lay["trans"].start] == M).all() and (got[:, lay["start"].start] == M).all() and (got[:, lay["end"].start] == M).all() and not gm.any()
    assert (got.sum(1) == 3 * M).all()
    M = 65600
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    chars = np.full((2, M), ord("x"), np.uint8)
    lens = np.array([M, M - 3], np.uint32)
    for form in ("pm-in", "sm"):
        rows = Rows(cfg, form, chars, lens)
        assert (rows.st.cpu().numpy() & 0xff == 0).all()
        got, gm = same_as_host(rows)
        assert got[0].max() >= M - 2 > 65535 and got[1].max() >= M - 5 and not gm.any()


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
def test_tampered_rows(form):
    """one mutation per string on the device copy of the rows (states, ids, flags, a flag bit above the two, at tile-edge rows): counts and misses are the host
    twin's of the same bytes, and misses is nonzero exactly where the device verdict has a lookup bit"""
    M = 264
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    chars, lens, muts = tamper_batch(M)
    rows = Rows(cfg, form, chars, lens)
    got, gm = same_as_host(rows)
    assert not gm.any()
    for b, m in enumerate(muts):
        if m is not None and m[0] != "mask":
            kind, r, d = m
            rows.xor_rec(b, r, d, {"state": 1, "first": 1, "sid": 1 << 16, "se": 1 << 24, "ee": 1 << 25, "fl4": 1 << 26}[kind])
    rows.xor_rec(0, 5, 1, 0xffff)                # out of range: a state, an id with its start flag, everything
    rows.xor_rec(1, 7, 0, 0x01ff0000)
    rows.xor_rec(len(muts) - 1, 30, 0, 0xffffffff)
    got, gm = same_as_host(rows)
    verdict = rows.verify()
    has_bit = (verdict & np.uint64(LOOKUP_BITS)) != 0
    assert np.array_equal(gm != 0, has_bit) and has_bit.sum() > 10 and (~has_bit).sum() > 10
    assert gm[0] and gm[1] and gm[len(muts) - 1] >= 2      # (row 30's state is out of range: its own transition lookup and that of row 29 miss)


def small_rows(form="pm-in", M=64, B=70, cfg=None):
    cfg = cfg or hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    chars, lens = batch(B, M)
    return Rows(cfg, form, chars, lens)


def test_capture_replay_and_a_side_stream():
    """a fresh context inside a capture: HRX_ERR_STATE and nothing written; after one eager call the launch captures, and replays into re-poisoned buffers"""
    rows = small_rows()
    cfg, B, W = rows.cfg, rows.B, rows.cfg.lookup_words()
    raw, flat = guarded(B * W)
    rawm, mo = guarded(B)
    side = torch.cuda.Stream(DEV)
    call = lambda: cfg.lookup_counts(rows.src, rows.d_lens, rows.rec, layout=rows.layout, out=flat.view(B, W), misses=mo, stream=side, **rows.kw)
    dummy = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                 # no lookup call before this one
        dummy.add_(1)
        with pytest.raises(hra.HrxError) as e:
            call()
    assert e.value.code == hra.HRX_ERR_STATE
    g.replay()
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((rawm == POISON).all())
    want, wm = host_counts(rows)
    got, gm = device_counts(rows, stream=side)             # the eager call, on a side stream: builds and uploads the image
    assert np.array_equal(got, want) and np.array_equal(gm, wm)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        call()
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((rawm == POISON).all())       # captured, not run
    for _ in range(2):
        g2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(flat.view(B, W).cpu().numpy().view(np.uint32), want) and np.array_equal(mo.cpu().numpy().view(np.uint32), wm)
        assert intact(raw, B * W) and intact(rawm, B)
        flat.fill_(POISON)
        mo.fill_(POISON)


def test_refused_calls_write_nothing():
    import ctypes as C
    rows = small_rows(form="planes")
    cfg, B, M, W = rows.cfg, rows.B, rows.M, rows.cfg.lookup_words()
    raw, flat = guarded(B * W)
    rawm, mo = guarded(B)
    lib, ctx = hra.lib, cfg._ctx
    arr = (C.c_void_p * 2)(*[p.data_ptr() for p in rows.planes])
    common = (rows.src.data_ptr(), rows.stride, rows.d_lens.data_ptr())
    f = lib.hrx_lookup_counts_device_planes
    tail = (flat.data_ptr(), mo.data_ptr(), None)
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, flat.data_ptr() + 4, mo.data_ptr(), None) == hra.HRX_ERR_ARG        # counts not 16-byte aligned
    assert f(ctx, hra.LAYOUT_STRING_MAJOR, *common, arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 1, B, M, 0, B, *tail) == hra.HRX_ERR_ARG                                            # wrong plane count
    assert f(ctx, PM, *common, arr, 3, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    null = (C.c_void_p * 2)(rows.planes[0].data_ptr(), None)
    assert f(ctx, PM, *common, null, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, None, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 2, B, (1 << 24) + 1, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 2, B, M, 1, B, *tail) == hra.HRX_ERR_ARG                                            # window past the batch
    assert f(ctx, PM, *common, arr, 2, B, M, B + 1, 0, *tail) == hra.HRX_OK                                             # (an empty window: no work)
    assert f(ctx, PM, rows.src.data_ptr() + 4, *common[1:], arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, None, mo.data_ptr(), None) == hra.HRX_ERR_ARG
    sm = small_rows(form="sm", cfg=cfg)
    args = (sm.src.data_ptr(), sm.stride, sm.d_lens.data_ptr(), sm.rec.data_ptr())
    h = lib.hrx_lookup_counts_device
    assert h(ctx, 0, *args, M - 1, B, M, 0, B, *tail) == hra.HRX_ERR_ARG                                                # pitch < M
    assert h(ctx, 4, *args, 0, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert h(ctx, 0, *args[:3], None, 0, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=hra.HRX_DEVICE_NONE)
    assert h(host_only._ctx, 0, *args, 0, B, M, 0, B, *tail) == hra.HRX_ERR_HIP
    assert f(host_only._ctx, PM, *common, arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((rawm == POISON).all())
    want, wm = host_counts(sm)
    assert h(ctx, 0, *args, 0, B, M, 0, B, flat.data_ptr(), None, None) == hra.HRX_OK                                   # misses may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(flat.view(B, W).cpu().numpy().view(np.uint32), want) and intact(raw, B * W) and bool((rawm == POISON).all())
    # a clone builds an image of its own at its first call
    got, gm = device_counts(sm, cfg=cfg.clone())
    assert np.array_equal(got, want) and np.array_equal(gm, wm)
