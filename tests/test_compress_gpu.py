"""LOOKUP COMPRESS on the device (hrx_lookup_compress_inputs_device / _planes, hrx_lookup_compress_table_device; csrc/hrx_kernel_compress.hip).  The rows come
from the device witness entry points; the yardsticks are the host twins (hrx_lookup_compress_inputs_host over the same rows copied to the host,
hrx_lookup_compress_table_host), limb for limb, and tests/compress_ref.py on a sample of strings — neither is the kernel under test.

  forms and shapes     sm, sm-pitched, pm, pm-in, planes (one def: the two row stripes) x 1, 5, 19, 72 rows and the kernel's rows per store instruction, per tile
                       and per workgroup, each - 1, + 0, + 1; 70 strings; one and two defs
  theta and flags      one challenge per string and one for the call; Montgomery and canonical limbs; values of r and more
  big states, defs     sweep_def(2045): states up to 2046; five and eight defs
  block border         65536 + 300 strings x 8 and x 19 rows: windows across the position-major block border and the launch cut at 32768 strings
  out of contract      lens = M + 1 (zero cells) and a byte without a transition beside untouched neighbours
  table                1, 3 and 70 runs per def set; the synthetic 256-state DFA's 65537 transition rows
  contract             capture and replay with theta rewritten between replays, a side stream, the first table call inside a capture, a host-only context

Every cells buffer lies between two poisoned 4-KiB guards.  No test provokes a fault: out-of-range values are folded, never used as addresses."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fr_cases as fc
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from compress_ref import CompressRef, R, limbs_of
from oracle_lib import OracleDefs
from test_match_cpu import CFG_H4, CFG_23
from test_verify_gpu import Rows, defs_of_files, defs_of_text, CFG_1, CFG_A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FORMS = ("sm", "sm-pitched", "pm", "pm-in", "planes")
# how compress_inputs_kernel cuts the rows (csrc/hrx_compress.hpp): kCzRowsPerStore rows per store instruction of a wave, kCzRowsPerTile per tile of a
# workgroup, at most kCzMaxTiles tiles per workgroup
ROWS_PER_STORE, ROWS_PER_TILE, MAX_TILES = 32, 512, 8
ROWS_PER_GROUP = ROWS_PER_TILE * MAX_TILES
LAUNCH_CUT = 32768            # strings per launch

_rng = np.random.default_rng(21)
T_RANDOM = int.from_bytes(_rng.bytes(32), "little") % R
EDGE_THETAS = [0, 1, R - 1, T_RANDOM, T_RANDOM + R, (1 << 256) - 1]


def thetas_for(count, seed=5):
    """(count, 4) uint64: the six edge values first (values of r and more among them), then seeded 256-bit values"""
    rng = np.random.default_rng(seed)
    vals = [EDGE_THETAS[i] if i < len(EDGE_THETAS) else int.from_bytes(rng.bytes(32), "little") for i in range(count)]
    return np.array([limbs_of(v) for v in vals], np.uint64), vals


def on_device(theta):
    return torch.from_numpy(np.ascontiguousarray(theta).view(np.int64)).to(DEV)


def device_cells(rows, theta, b_begin=0, b_count=None, canonical=False, stream=None):
    """the device cells of a window between their guards, as uint64 [3 D][b_count][M][4]; theta: uint64 limbs (b_count, 4) or (4,)"""
    b_count = rows.B - b_begin if b_count is None else b_count
    cells, raw = fc.guarded_cells(torch, DEV, 3 * rows.D, b_count, rows.M)
    out = rows.cfg.lookup_compress_inputs(rows.src, rows.d_lens, rows.rec, on_device(theta), layout=rows.layout, planes=rows.planes, b_begin=b_begin, b_count=b_count,
                                          out=cells, canonical=canonical, stream=stream, **rows.kw)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert out.data_ptr() == cells.data_ptr()
    fc.guards_intact(raw, cells, rows.form)
    return cells.cpu().numpy().view(np.uint64)


def host_cells(rows, theta, b_begin=0, b_count=None, canonical=False):
    rec, msk = rows.host_rows()
    return rows.cfg.lookup_compress_inputs_host(rows.chars, rows.lens, rec, theta, b_begin=b_begin, b_count=b_count, canonical=canonical)


def same_as_host(rows, theta, b_begin=0, b_count=None, canonical=False):
    got = device_cells(rows, theta, b_begin, b_count, canonical)
    want = host_cells(rows, theta, b_begin, b_count, canonical)
    assert fc.first_difference(got, want) is None, "%s B=%d M=%d window %d+%s canonical=%s: %s" % (rows.form, rows.B, rows.M, b_begin, b_count, canonical,
                                                                                                fc.first_difference(got, want))
    return got


def against_ref(rows, ref, got, vals, sample, canonical, b_begin=0):
    """vals: the challenge of the call, or one per string of the window"""
    rec, msk = rows.host_rows()
    for b in sample:
        th = vals if isinstance(vals, int) else vals[b - b_begin]
        want = ref.cells_of_records(rows.chars[b], int(rows.lens[b]), rows.M, rec[b], th, canonical)
        assert np.array_equal(got[:, b - b_begin], want), (rows.form, b, canonical)


def batch(B, M, seed=3):
    chars, lens = synth.ragged(B, M, seed=seed)
    lens = np.minimum(lens, M).astype(np.uint32)
    if B > 2:
        lens[0], lens[1] = 0, M
    return np.ascontiguousarray(chars), lens


def all_modes(rows, ref, sample):
    """per-string and shared challenges, Montgomery and canonical, against the host twin; the yardstick on a sample"""
    th, vals = thetas_for(rows.B)
    got = same_as_host(rows, th)
    same_as_host(rows, th[4], canonical=True)                      # one challenge for the call: T_RANDOM + r, canonical
    if ref is not None:
        against_ref(rows, ref, got, vals, sample, False)
        got = same_as_host(rows, th, canonical=True)
        against_ref(rows, ref, got, vals, sample, True)
        got = same_as_host(rows, th[3])
        against_ref(rows, ref, got, vals[3], sample, False)


@pytest.mark.parametrize("M", [1, 5, 19, 72, ROWS_PER_STORE - 1, ROWS_PER_STORE, ROWS_PER_STORE + 1, ROWS_PER_TILE - 1, ROWS_PER_TILE, ROWS_PER_TILE + 1])
@pytest.mark.parametrize("names", [CFG_1, CFG_A], ids=["D1", "D2"])
def test_every_form_and_shape(oracle, names, M):
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0)
    ref = CompressRef(OracleDefs.from_files(oracle, names))
    chars, lens = batch(70, M, seed=M)
    for form in FORMS:
        rows = Rows(cfg, form, chars, lens)
        all_modes(rows, ref if form in ("sm", "pm-in") and M <= 72 else None, [0, 1, 35, 69])


@pytest.mark.parametrize("M", [ROWS_PER_GROUP - 1, ROWS_PER_GROUP, ROWS_PER_GROUP + 1])
def test_around_the_rows_of_a_workgroup(M):
    """the most rows one workgroup serves, - 1 and + 1: with one more a string has two workgroups, the second with one row"""
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    chars, lens = batch(6, M, seed=M)
    lens[2] = M - 1
    for form in ("sm", "pm-in", "planes"):
        rows = Rows(cfg, form, chars, lens)
        th, vals = thetas_for(rows.B)
        same_as_host(rows, th)


@pytest.mark.parametrize("D", [1, 2])
def test_big_states(oracle, D):
    """sweep_def: states up to 2046 (one def) — every component of a tuple beyond 8 bits, the dummy state beyond 10"""
    defs_t = fc.sweep_defs(D)
    L = fc.SWEEP_L if D == 1 else fc.SWEEP_L2
    chars, lens = fc.sweep_batch(L)
    cfg = hra.RegexVerifyConfig.configure(72, defs_of_text(defs_t), device=0)
    ref = CompressRef(OracleDefs(oracle, [(t[0].encode(), [s.encode() for s in t[1]]) for t in defs_t]))
    for form in FORMS:
        rows = Rows(cfg, form, chars, lens)
        assert max(int(x) & 0xffff for x in rows.host_rows()[0].reshape(-1)) >= (2000 if D == 1 else 1000)
        all_modes(rows, ref if form == "pm-in" else None, [0, 17, 31, 39])


@pytest.mark.parametrize("name,names", [("five", CFG_H4 + CFG_23[:1]), ("eight", CFG_H4 * 2)])
def test_five_and_eight_defs(oracle, name, names):
    M = 64
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0)
    ref = CompressRef(OracleDefs.from_files(oracle, names))
    chars, lens = batch(70, M, seed=70)
    for form in ("sm", "pm-in", "planes"):
        rows = Rows(cfg, form, chars, lens)
        all_modes(rows, ref if form == "pm-in" else None, [0, 1, 69])


@pytest.mark.parametrize("form", ["pm", "pm-in"])
@pytest.mark.parametrize("tall", [False, True], ids=["8rows", "19rows"])
def test_block_border_and_launch_cut(oracle, form, tall):
    """65536 + 300 strings of sweep_def(40): windows across the position-major block border (the second block's string count enters every index) and across
    the cut of a call into launches of 32768 strings — theta, the cells and the strings advance together"""
    chars, lens = fc.tall_batch() if tall else fc.big_batch(alphabet=fc.BIG_SWEEP_BYTES)
    M = fc.TALL_M if tall else fc.BIG_M
    defs_t = [fc.sweep_def(fc.BIG_SWEEP_L)]
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(defs_t), device=0)
    rows = Rows(cfg, form, chars, lens)
    ref = CompressRef(OracleDefs(oracle, [(defs_t[0][0].encode(), [s.encode() for s in defs_t[0][1]])]))
    for b_begin, b_count in ((65400, 300), (65535, 2), (30000, 35800)):
        assert b_begin < hra.PM_BLOCK < b_begin + b_count
        th, vals = thetas_for(b_count, seed=b_count)
        got = same_as_host(rows, th, b_begin, b_count)
        edges = sorted({b_begin, hra.PM_BLOCK - 1, hra.PM_BLOCK, b_begin + b_count - 1} | ({b_begin + LAUNCH_CUT - 1, b_begin + LAUNCH_CUT} if b_count > LAUNCH_CUT else set()))
        against_ref(rows, ref, got, vals, edges, False, b_begin=b_begin)
    same_as_host(rows, thetas_for(4)[0][3], 30000, 35800, canonical=True)


def test_out_of_contract_strings():
    """lens = M + 1: the string has no rows, zero cells; a byte without a transition: the cells of whatever rows the witness launch left, as the host twin
    folds them; every other string's cells as if the three were not there"""
    M = 72
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(fc.CFG_A), device=0)
    chars, lens = fc.bad_batch(M)
    good_chars, good_lens = fc.defcount_batch(fc.CFG_A, 70, M)
    others = [b for b in range(70) if b not in fc.BAD_STRINGS]
    th, vals = thetas_for(70)
    for form in ("sm", "pm-in", "planes"):
        rows = Rows(cfg, form, chars, lens)
        got = same_as_host(rows, th)
        assert not got[:, 3].any() and not got[:, 40].any() and got[:, 9].any()
        clean = device_cells(Rows(cfg, form, good_chars, good_lens), th)
        assert np.array_equal(got[:, others], clean[:, others])


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------
def device_table(cfg, theta, canonical=False, stream=None):
    n_theta, W = (1 if theta.ndim == 1 else len(theta)), cfg.lookup_words()
    cells, raw = fc.guarded_cells(torch, DEV, 1, n_theta, W)
    out = cfg.lookup_compress_table(on_device(theta), out=cells.view(n_theta, W, 4), canonical=canonical, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert out.data_ptr() == cells.data_ptr()
    fc.guards_intact(raw, cells, "table")
    return cells.cpu().numpy().view(np.uint64)[0]


@pytest.mark.parametrize("name", ["regex12", "five", "eight", "sweep"])
def test_table_cells(oracle, name):
    if name == "sweep":
        defs_t = fc.sweep_defs(1)
        cfg = hra.RegexVerifyConfig.configure(64, defs_of_text(defs_t), device=0)
        ref = CompressRef(OracleDefs(oracle, [(t[0].encode(), [s.encode() for s in t[1]]) for t in defs_t]))
    else:
        names = {"regex12": CFG_A, "five": CFG_H4 + CFG_23[:1], "eight": CFG_H4 * 2}[name]
        cfg = hra.RegexVerifyConfig.configure(64, defs_of_files(names), device=0)
        ref = CompressRef(OracleDefs.from_files(oracle, names))
    lay = cfg.lookup_layout()
    for n_theta in (1, 3, 70):
        th, vals = thetas_for(n_theta)
        for canonical in (False, True):
            got = device_table(cfg, th, canonical)
            assert np.array_equal(got, cfg.lookup_compress_table_host(th, canonical=canonical)), (name, n_theta, canonical)
            assert not got[:, lay[-1]["end"].stop:].any()
            for k in sorted({0, n_theta // 2, n_theta - 1}):
                assert np.array_equal(got[k], ref.table_cells(vals[k], canonical))
    one = device_table(cfg, thetas_for(4)[0][3])
    assert one.shape[0] == 1 and np.array_equal(one[0], ref.table_cells(T_RANDOM, False))


def test_table_of_the_synthetic_256_state_dfa(oracle):
    """65537 transition rows: 65 workgroups a run, the last with one row"""
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    cfg = hra.RegexVerifyConfig.configure(64, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=0)
    assert cfg.lookup_layout()[0]["trans"].stop == 65537
    th, vals = thetas_for(2)
    th, vals = th[::-1].copy(), vals[::-1]
    got = device_table(cfg, th)
    assert np.array_equal(got, cfg.lookup_compress_table_host(th))
    enc = lambda t: t.encode() if isinstance(t, str) else t
    ref = CompressRef(OracleDefs(oracle, [(enc(a_txt), [enc(sub_txt)])]))
    assert np.array_equal(got[0], ref.table_cells(vals[0], False))


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
def test_capture_replay_with_theta_rewritten_and_a_side_stream():
    """the compress calls over rows read no image: a fresh context captures at its first call; the cells follow what theta holds at each replay.  The first
    table call inside a capture: HRX_ERR_STATE and nothing written; after one eager call it captures too"""
    M, B = 64, 70
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    chars, lens = batch(B, M)
    rows = Rows(cfg, "pm-in", chars, lens)
    W = cfg.lookup_words()
    cells, raw = fc.guarded_cells(torch, DEV, 3 * rows.D, B, M)
    tcells, traw = fc.guarded_cells(torch, DEV, 1, 1, W)
    th, vals = thetas_for(B)
    d_theta = on_device(th)
    side = torch.cuda.Stream(DEV)
    call = lambda: cfg.lookup_compress_inputs(rows.src, rows.d_lens, rows.rec, d_theta, layout=rows.layout, out=cells, stream=side, **rows.kw)
    table_call = lambda: cfg.lookup_compress_table(d_theta[:1], out=tcells.view(1, W, 4), stream=side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                 # no compress call before these
        call()
        with pytest.raises(hra.HrxError) as e:
            table_call()
    assert e.value.code == hra.HRX_ERR_STATE
    torch.cuda.synchronize()
    assert fc.untouched(raw) and fc.untouched(traw)        # captured, not run
    for seed in (5, 6):
        th, vals = thetas_for(B, seed=seed)
        th = np.roll(th, seed, axis=0)
        d_theta.copy_(on_device(th))
        g.replay()
        torch.cuda.synchronize()
        assert fc.first_difference(cells.cpu().numpy().view(np.uint64), host_cells(rows, th)) is None
        fc.guards_intact(raw, cells, "replay")
        assert fc.untouched(traw)
    got = device_table(cfg, th[:1], stream=side)           # the eager call, on a side stream: builds and uploads the tuples
    assert np.array_equal(got, cfg.lookup_compress_table_host(th[:1]))
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        table_call()
    torch.cuda.synchronize()
    assert fc.untouched(traw)
    g2.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tcells.cpu().numpy().view(np.uint64)[0], got)
    fc.guards_intact(traw, tcells, "table replay")
    # the eager call on the side stream
    assert fc.first_difference(device_cells(rows, th, stream=side), host_cells(rows, th)) is None


def test_refused_calls_write_nothing():
    import ctypes as C
    M, B = 64, 70
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    chars, lens = batch(B, M)
    rows = Rows(cfg, "planes", chars, lens)
    cells, raw = fc.guarded_cells(torch, DEV, 3, B, M)
    d_theta = on_device(thetas_for(B)[0])
    lib, ctx = hra.lib, cfg._ctx
    PM = hra.LAYOUT_POSITION_MAJOR
    arr = (C.c_void_p * 2)(*[p.data_ptr() for p in rows.planes])
    common = (rows.src.data_ptr(), rows.stride, rows.d_lens.data_ptr())
    f = lib.hrx_lookup_compress_inputs_device_planes
    tail = (d_theta.data_ptr(), 4, cells.data_ptr(), 0, None)
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, d_theta.data_ptr(), 2, cells.data_ptr(), 0, None) == hra.HRX_ERR_ARG           # theta_stride
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, d_theta.data_ptr(), 4, cells.data_ptr() + 8, 0, None) == hra.HRX_ERR_ARG       # cells not 16-byte aligned
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, d_theta.data_ptr() + 4, 4, cells.data_ptr(), 0, None) == hra.HRX_ERR_ARG       # theta not 8-byte aligned
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, d_theta.data_ptr(), 4, cells.data_ptr(), 2, None) == hra.HRX_ERR_ARG           # unknown flag bits
    assert f(ctx, hra.LAYOUT_STRING_MAJOR, *common, arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG                                 # planes, string-major
    assert f(ctx, PM, *common, arr, 3, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, None, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 2, B, M, 1, B, *tail) == hra.HRX_ERR_ARG                                                      # a window behind the batch
    assert f(ctx, PM, *common, arr, 2, B, M, B + 1, 0, *tail) == hra.HRX_OK                                                       # (an empty window: no work)
    assert f(ctx, PM, rows.src.data_ptr() + 4, *common[1:], arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_ARG
    assert f(ctx, PM, *common, arr, 2, B, M, 0, B, None, 4, cells.data_ptr(), 0, None) == hra.HRX_ERR_ARG
    t = lib.hrx_lookup_compress_table_device
    assert t(ctx, d_theta.data_ptr(), 3, 2, cells.data_ptr(), 0, None) == hra.HRX_ERR_ARG
    assert t(ctx, d_theta.data_ptr(), 4, 2, cells.data_ptr() + 8, 0, None) == hra.HRX_ERR_ARG
    assert t(ctx, d_theta.data_ptr(), 4, 2, cells.data_ptr(), 8, None) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=hra.HRX_DEVICE_NONE)
    assert f(host_only._ctx, PM, *common, arr, 2, B, M, 0, B, *tail) == hra.HRX_ERR_HIP
    assert t(host_only._ctx, d_theta.data_ptr(), 4, 2, cells.data_ptr(), 0, None) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert fc.untouched(raw)
