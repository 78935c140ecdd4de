"""How a caller may behave, beyond what the other GPU tests do (helpers of tests/test_caller_conditions_cpu.py / _gpu.py; plain module, torch is passed in):

  MinAlign        an allocator that hands out every buffer at exactly the alignment include/hrx.h promises to accept (16, 8 or 4 bytes, never more),
                  between two poisoned guards of GUARD bytes: a prover that carves its buffers out of a pool of its own passes such pointers
  OnSideStream    a config whose device calls run the decoy protocol on a non-blocking side stream: inputs that hold the batch in reversed string
                  order until copies queued on that stream, behind a delay, overwrite them; a step of the library that left the caller's stream reads
                  the decoy or is overwritten
  the cases, seeds and row selections both test files use, so that what the CPU file asserts about them holds for what the GPU file runs."""
import dataclasses
import time

import numpy as np

import carry_defs as cd
import fuzz_defs as fd

GUARD = 4096
POISON = 0xA5
PM_BLOCK = 65536
# the contractual minimum alignment of every argument kind (include/hrx.h and the entries' argument checks)
MIN_ALIGN = {"chars": 16, "values": 16, "chars_pm": 16, "records": 16, "masked": 16, "plane": 16, "cells": 16, "chars_pm_out": 16,
             "status": 8, "status_in": 8, "offsets": 8, "spans": 8, "counts": 8, "workspace": 8, "run_offsets": 8, "runs": 8, "byte_offsets": 8, "totals": 8, "bucket_offsets": 8,
             "lens": 4, "sel": 4, "order": 4, "span_counts": 4, "lens_out": 4,
             "bytes_out": 1}          # (extract's values: no rule at all)
INPUT_KINDS = ("chars", "values", "chars_pm", "offsets", "lens", "sel", "status_in", "span_counts")


class MinAlign:
    """alloc(nbytes, dtype, kind) -> (view, raw): GUARD + a + nbytes + GUARD poisoned bytes on a 256-aligned base, the view at byte GUARD + a with a =
    MIN_ALIGN[kind], so its address is a multiple of a and of nothing more; raw: the bytes from the view's first one on (the view, then the guard behind
    it).  check() looks at both guards of every buffer handed out."""

    def __init__(self, torch, dev, poison=POISON):
        self.torch, self.dev, self.poison, self.bufs = torch, dev, poison, []

    def __call__(self, nbytes, dtype, kind):
        torch, a = self.torch, MIN_ALIGN[kind]
        whole = torch.full((GUARD + a + nbytes + GUARD,), self.poison, dtype=torch.uint8, device=self.dev)
        assert whole.data_ptr() % 256 == 0, "the allocator's own base"
        lo = GUARD + a
        view = whole[lo:lo + nbytes]
        assert (whole.data_ptr() + lo) % (2 * a) == a, (kind, whole.data_ptr() + lo)      # (an empty view has no address of its own)
        self.bufs.append((whole, lo, nbytes, kind))
        return view.view(dtype), whole[lo:]

    def outputs(self, since=0):
        return [b for b in self.bufs[since:] if b[3] not in INPUT_KINDS]

    def repoison(self, since=0):
        for whole, _, _, _ in self.outputs(since):
            whole.fill_(self.poison)

    def check(self, tag):
        for k, (whole, lo, nbytes, kind) in enumerate(self.bufs):
            for name, part in (("in front of", whole[:lo]), ("behind", whole[lo + nbytes:])):
                bad = (part != self.poison).nonzero()
                assert bad.numel() == 0, "%s: a write %s buffer %d (%s, %d bytes), guard byte %d" % (tag, name, k, kind, nbytes, int(bad[0]))

    def all_poison(self, since=0):
        return all(bool((whole == self.poison).all()) for whole, _, _, _ in self.outputs(since))


# ---- reversed string order: the decoy ---------------------------------------------------------------------------------------------------------------
def pm_chars_to_string_major(chars_pm, B, stride):
    """inverse of chars_to_position_major (torch)"""
    parts = []
    for k0 in range(0, B, PM_BLOCK):
        nb = min(PM_BLOCK, B - k0)
        parts.append(chars_pm[k0 * stride:(k0 + nb) * stride].view(stride // 16, nb, 16).permute(1, 0, 2).reshape(nb, stride))
    import torch
    return torch.cat(parts) if parts else chars_pm.reshape(0, stride)


def reversed_ragged(torch, values, offsets):
    """(values, offsets) of the same sizes that hold the strings in reversed order behind the same lead (decreasing offsets count as empty strings)"""
    v, o = values.cpu().numpy(), offsets.cpu().numpy().astype(np.int64)
    n = np.maximum(np.diff(o), 0)
    strings = [v[int(o[b]):int(o[b]) + int(n[b])] for b in range(len(n))][::-1]
    out = np.full(len(v), 0xAA, np.uint8)
    ro = np.zeros(len(o), np.int64)
    ro[0] = o[0]
    np.cumsum(n[::-1], out=ro[1:])
    ro[1:] += o[0]
    body = np.concatenate(strings) if strings else np.zeros(0, np.uint8)
    end = min(len(out), int(o[0]) + len(body))
    out[int(o[0]):end] = body[:end - int(o[0])]
    return torch.from_numpy(out).to(values.device), torch.from_numpy(ro).to(offsets.device)


class OnSideStream:
    """cfg seen through the decoy protocol.  Every wrapped device call, given stream=s (a fresh non-blocking torch stream):
      1. runs once, eagerly, on the current (default) stream, so that the context's scratch exists; device-wide synchronize
      2. its inputs are overwritten with the decoy X (the batch in reversed string order) and the call runs eagerly once more, so that the scratch holds the
         decoy's intermediate rows and not the right ones (a step that left the stream would else find the warm call's answer there); the outputs made
         since the last call are re-poisoned; synchronize
      3. on s: a delay (torch.cuda._sleep), an event, copies that put the real inputs Y back, the library call, copies of every output buffer (guards
         included) to pinned host memory
      4. `not event.query()` right after the library call returned: the call was asynchronous and the race window open — else the test FAILS
      5. s.synchronize() alone; the pinned copies must equal what the device buffers hold afterwards, which the caller then compares with the oracle.
    A launch, memset or copy of the library that went to another stream than s reads X, or is overwritten by the real launch's output, or lands after the
    copies: the comparison with the oracle's rows for Y fails.  returns[]: the host-side seconds each warm call and each side-stream call took to return."""

    INPUTS = {       # method -> how the decoy of its inputs is made
        "witness_batch": "padded", "witness_batch_position_major": "padded", "witness_batch_planes": "padded", "match_batch": "padded",
        "extract_batch": "padded", "match_batch_ragged": "ragged", "extract_batch_ragged": "ragged", "ragged_to_position_major": "ragged",
        "chars_to_position_major_device": "chars", "match_selected": "selected", "gather_to_position_major": "gathered", "route": "route",
        "fr_columns": "fr"}

    def __init__(self, torch, cfg, alloc, cycles):
        self._torch, self._cfg, self._alloc, self._cycles = torch, cfg, alloc, cycles
        self._mark = 0
        self.calls, self.returns = 0, []

    def __getattr__(self, name):
        real = getattr(self._cfg, name)
        if name not in self.INPUTS:
            return real
        return lambda *a, **kw: self._call(name, real, a, kw)

    # -- (tensor, decoy) pairs of a call's inputs
    def _pairs(self, name, a, kw):
        torch = self._torch
        how = self.INPUTS[name]
        if how == "chars":
            return [(a[0], a[0].flip(0))]
        if how == "padded":
            chars, lens = a[0], a[1]
            if kw.get("chars_pm_stride") is None:
                return [(chars, chars.flip(0)), (lens, lens.flip(0))]
            stride, B = int(kw["chars_pm_stride"]), lens.numel()
            import halo2_regex_amd as hra
            return [(chars, hra.chars_to_position_major(pm_chars_to_string_major(chars, B, stride).flip(0).contiguous())), (lens, lens.flip(0))]
        if how == "ragged":
            rv, ro = reversed_ragged(torch, a[0], a[1])
            return [(a[0], rv), (a[1], ro)]
        if how in ("selected", "gathered"):
            src, sel = a[0], a[1]
            if kw.get("offsets") is not None:
                rv, ro = reversed_ragged(torch, src, kw["offsets"])
                pairs, B = [(src, rv), (kw["offsets"], ro)], kw["offsets"].numel() - 1
            else:
                pairs, B = [(src, src.flip(0)), (kw["lens"], kw["lens"].flip(0))], kw["lens"].numel()
            s64 = sel.to(torch.int64) & 0xffffffff
            pairs.append((sel, torch.where(s64 < B, B - 1 - s64, s64).to(torch.int32)))          # other strings than the call's own
            return pairs
        if how == "route":
            pairs = [] if a[0] is None else [(a[0], a[0].flip(0))]
            if kw.get("lens") is not None:
                pairs.append((kw["lens"], kw["lens"].flip(0)))
            else:
                o = kw["offsets"]
                n = (o[1:] - o[:-1]).flip(0)
                pairs.append((o, torch.cat([o[:1], o[0] + torch.cumsum(n, 0)])))
            return pairs
        assert how == "fr"
        chars, lens, (rec, msk, _) = a[0], a[1], a[2]
        if kw.get("chars_pm_stride") is None:
            pairs = [(chars, chars.flip(0))]
        else:
            import halo2_regex_amd as hra
            pairs = [(chars, hra.chars_to_position_major(pm_chars_to_string_major(chars, lens.numel(), int(kw["chars_pm_stride"])).flip(0).contiguous()))]
        pairs.append((lens, lens.flip(0)))
        for t in (list(rec) if isinstance(rec, (list, tuple)) else [rec]) + [msk]:      # the rows the cells are made of: no rows at all
            pairs.append((t, torch.zeros_like(t)))
        return pairs

    def _call(self, name, real, a, kw):
        torch = self._torch
        kw = dict(kw)
        s = kw.pop("stream", None)
        assert s is not None and s != torch.cuda.current_stream(), "the protocol needs a side stream"
        t0 = time.perf_counter()
        real(*a, **kw)                                   # 1. eager, on the current stream: the scratch exists from here on
        warm = time.perf_counter() - t0
        torch.cuda.synchronize()
        pairs = self._pairs(name, a, kw)
        ys = [t.clone() for t, _ in pairs]
        for t, x in pairs:                               # 2. the decoy in, and through the library once: the scratch holds the decoy's rows; poison over the outputs
            assert x.shape == t.shape and x.dtype == t.dtype, name
            t.copy_(x)
        real(*a, **kw)
        outs = self._alloc.outputs(self._mark)
        self._alloc.repoison(self._mark)
        self._mark = len(self._alloc.bufs)
        pinned = [torch.empty(w.shape, dtype=w.dtype, device="cpu").pin_memory() for w, _, _, _ in outs]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):                       # 3.
            torch.cuda._sleep(self._cycles)
            ev = torch.cuda.Event()
            ev.record(s)
            for (t, _), y in zip(pairs, ys):
                t.copy_(y, non_blocking=True)
            t0 = time.perf_counter()
            r = real(*a, stream=s, **kw)
            side = time.perf_counter() - t0
            window_open = not ev.query()                 # 4.
            for p, (w, _, _, _) in zip(pinned, outs):
                p.copy_(w, non_blocking=True)
        assert window_open, "%s: the delay had ended when the call returned (%.3f ms on the host): the race window was not open" % (name, side * 1e3)
        s.synchronize()                                  # 5. this stream alone
        for k, (p, (w, _, _, kind)) in enumerate(zip(pinned, outs)):
            assert torch.equal(p, w.cpu()), "%s: output %d (%s) changed after the copies queued behind the call on its stream" % (name, k, kind)
        self.calls += 1
        self.returns.append((name, warm, side))
        return r


def launch_form(hra, torch, cfg, form, src_chars, src_lens, M, D, alloc, stream=None, defer=False):
    """One witness launch and nothing else: src_chars (B, stride) uint8 and src_lens (B,) int32, device tensors, copied into the allocator's buffers (by
    torch's current stream, which the caller makes `stream`), the launch on `stream`, no synchronization.  form: sm / sm-pitched (witness_batch),
    pm / pm-in (witness_batch_position_major from string-major / position-major input), planes / planes-in (witness_batch_planes: record planes, two row
    stripes at one def).  Returns read() -> (status (B,), records (B, M, D), masked (B, M)) numpy, to be called once the stream is done (it checks the
    pitch gaps of the pitched form); defer: nothing is launched yet, returns (go, read) — go() makes the library call and nothing else."""
    import ctypes as C
    B, stride = src_chars.shape
    skw = {} if stream is None else dict(stream=stream)
    c = alloc(B * stride, torch.uint8, "chars")[0].view(B, stride)
    l = alloc(B * 4, torch.int32, "lens")[0]
    c.copy_(src_chars)
    l.copy_(src_lens)
    src, kw = c, {}
    if form.endswith("-in"):
        src, kw = alloc(B * stride, torch.uint8, "chars_pm")[0], dict(chars_pm_stride=stride)
        src.copy_(hra.chars_to_position_major(c))
    empty = (np.zeros(0, np.uint64), np.zeros((0, M, D), np.uint32), np.zeros((0, M), np.uint16))
    if form.startswith("sm"):
        rp, mp = hra.recommended_pitches(M)[:2] if form == "sm-pitched" else (M, M)
        r_v, r_raw = alloc(B * rp * D * 4, torch.int32, "records")
        m_v, m_raw = alloc(B * mp * 2, torch.int16, "masked")
        s_v = alloc(B * 8, torch.int64, "status")[0]
        out = (r_v.view(B, rp, D)[:, :M], m_v.view(B, mp)[:, :M], s_v)
        def go():
            cfg.witness_batch(c, l, out=out, **skw)

        def read():
            if rp > M or mp > M:
                assert (r_raw[:B * rp * D * 4].view(B, rp, D * 4)[:, M:] == alloc.poison).all(), "a write into the records' pitch gap"
                assert (m_raw[:B * mp * 2].view(B, mp, 2)[:, M:] == alloc.poison).all(), "a write into the masked rows' pitch gap"
            return out[2].cpu().numpy().view(np.uint64), out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(np.uint16)
        return (go, read) if defer else (go(), read)[1]
    if form.startswith("pm"):
        nr, nm = C.c_size_t(0), C.c_size_t(0)
        hra.lib.hrx_position_major_sizes(B, M, D, C.byref(nr), C.byref(nm))
        r_v, m_v, s_v = alloc(nr.value * 4, torch.int32, "records")[0], alloc(nm.value * 2, torch.int16, "masked")[0], alloc(B * 8, torch.int64, "status")[0]
        def go():
            cfg.witness_batch_position_major(src, l, out=(r_v, m_v, s_v), **kw, **skw)

        def read():
            if B == 0:
                return empty
            r1, m1 = hra.position_major_to_string_major(r_v, m_v, B, M, D)
            return s_v.cpu().numpy().view(np.uint64), r1.cpu().numpy().view(np.uint32), m1.cpu().numpy().view(np.uint16)
        return (go, read) if defer else (go(), read)[1]
    assert form.startswith("planes"), form
    R = 2 if D == 1 else 1
    npl, nmp = C.c_size_t(0), C.c_size_t(0)
    hra.lib.hrx_position_major_stripe_sizes(B, M, R, C.byref(npl), C.byref(nmp))
    planes = [alloc(npl.value * 4, torch.int32, "plane")[0] for _ in range(D * R)]
    m_v, s_v = alloc(nmp.value * 2, torch.int16, "masked")[0], alloc(B * 8, torch.int64, "status")[0]
    def go():
        cfg.witness_batch_planes(src, l, out=(planes, m_v, s_v), **kw, **skw)

    def read():
        if B == 0:
            return empty
        r1, m1 = hra.planes_to_string_major(planes, m_v, B, M, D)
        return s_v.cpu().numpy().view(np.uint64), r1.cpu().numpy().view(np.uint32), m1.cpu().numpy().view(np.uint16)
    return (go, read) if defer else (go(), read)[1]


def calibrate_delay(torch, want_ms=25.0):
    """(cycles, measured ms): torch.cuda._sleep cycles for a delay of about want_ms, from one timed probe, and the timed delay itself"""
    def timed(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    timed(1000)
    probe = 2_000_000
    ms = max(timed(probe), 1e-3)
    cycles = int(min(max(probe * want_ms / ms, 1_000_000), 4_000_000_000))
    return cycles, timed(cycles)


# ---- the cases both files use -----------------------------------------------------------------------------------------------------------------------
CHUNK_ROW_ID = "chunked"
SCRATCH_ROWS = (CHUNK_ROW_ID, "pm-multi-pass-merge", "pm-multi-pass-combine", "sm-via-pm-half", "pm-dynamic-groups",        # the witness paths that own context scratch
                # string-major outputs of four and more defs, one row of each route: group-private records behind the copy-mode combine; position-major scratch and the
                # transposer behind the class-wide launch, behind class-wide groups with the summary combine, and behind groups of three merged by the last pass
                "sm-multi-pass-copy-combine", "sm-class-wide-transpose", "sm-class-wide-groups-transpose", "sm-multi-pass-merge-transpose")
SEQUENCE_ROWS = SCRATCH_ROWS + ("pm-narrow", "pm-class-def-parallel", "sm-split-4byte")
SEQUENCE_SIZES = (129, 1, 65, 320, 64, 129, 0)


def chunk_row():
    from test_carry_gpu import _chunk_row
    return _chunk_row("chunked=%dx4 tiles" % (cd.WITNESS_M // cd.FORCED_CHUNK), 0x80)


def chunk_case(D):
    """the lever batch of the forced chunked launch (M = 2048, chunks of cd.FORCED_CHUNK rows); every 29th string claims M + 1 bytes (status 3, which the
    lever batches do not hold themselves).  seed: odd at D = 1 (string-major input to the planes launch), even at D = 2"""
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, D=D)
    case.lens = case.lens.copy()
    case.lens[7::29] = case.M + 1
    case.seed = D
    return case


def chunk_revealing_case(D=2, repeat=1):
    """chunk_case's strings that the oracle has something to say about — a confirmed range (revealed rows), a bad status, a claimed length of M + 1 —, about a
    quarter of the lever batch (in most of its strings the range is taken back and nothing is revealed: a decoy of such strings bites nowhere); repeat > 1:
    that many copies, every 7th string of the copies with the byte no def has a transition for (status 1) in its middle"""
    case = chunk_case(D)
    keep = [b for b in range(case.B) if any(k == "confirmed" for _, _, k in case.ranges[b]) or case.want[b] != 0 or case.lens[b] > case.M]
    case.chars, case.lens, case.want, case.B = np.tile(case.chars[keep], (repeat, 1)), np.tile(case.lens[keep], repeat), np.tile(case.want[keep], repeat), len(keep) * repeat
    case.ranges, case.names = [case.ranges[i] for i in keep] * repeat, [case.names[i] for i in keep] * repeat
    for b in range(len(keep), case.B, 7):
        if 2 <= case.lens[b] <= case.M:
            case.chars[b, int(case.lens[b]) // 2] = cd.UNDEF
    case.seed = D + 2 * repeat
    return case


def all_rows():
    from test_variants_gpu import ROWS
    return list(ROWS) + [chunk_row()]


def row_of(row_id):
    return [r for r in all_rows() if r["id"] == row_id][0]


def _row_cases(row):
    from test_variants_gpu import SEEDS
    if row["id"] == CHUNK_ROW_ID:
        return [chunk_case(1), chunk_case(2)]
    return [fd.make_case(s, row["shape"]) for s in row.get("seeds", SEEDS)]


def alignment_cases(row):
    """two of the row's cases: one whose M is no multiple of 8 where the row has one (with more than one string if possible), one whose B is no multiple of
    64 (the largest); and the case the row's fr_columns check runs on, where it has one"""
    from test_variants_gpu import fr_case
    cases = _row_cases(row)
    odd = [c for c in cases if c.M % 8] or cases
    first = ([c for c in odd if c.B > 1] or odd)[0]
    rest = [c for c in cases if c is not first and c.B % 64]
    picked = [first] + ([max(rest, key=lambda c: (c.B, c.M))] if rest else [])
    fr_seed = fr_case(row, cases) if row.get("fr") else None
    if fr_seed is not None and fr_seed not in [c.seed for c in picked]:
        picked.append([c for c in cases if c.seed == fr_seed][0])
    return picked, fr_seed


def stream_case(row):
    """the row's case for the side-stream runs: many strings, no multiple of 64, the most rows"""
    if row["id"] == CHUNK_ROW_ID:
        return chunk_revealing_case(2)
    cases = [c for c in _row_cases(row) if c.B % 64]
    return max(cases, key=lambda c: (c.B > 1, c.M >= 16, c.B, c.M))


def sequence_case(row):
    """the row's batch for the long-lived context: seed 4 (129 strings) repeated to about 320 (more where the row's variant needs more)"""
    if row["id"] == CHUNK_ROW_ID:
        return chunk_revealing_case(2, repeat=4)
    sh = row["shape"]
    return fd.make_case(4, dataclasses.replace(sh, min_batch=max(320, sh.min_batch)))


def sequence_sizes(row, case):
    """SEQUENCE_SIZES; a row whose variant needs min_batch strings takes its whole batch where the others take 320"""
    big = case.B if row["id"] != CHUNK_ROW_ID and row["shape"].min_batch > 320 else 320
    return tuple(big if n == 320 else n for n in SEQUENCE_SIZES)


def selection(case, ost, omsk, k, n):
    """the k-th call's n strings of the case: a permutation (seeded by k) whose first accepted string that reveals something, first string of status 1 and
    first of status 3 are moved to its front, then its first n — so a selection of ONE string is such an accepted one, and every larger one holds all three
    (ost, omsk: the oracle's status words and masked rows, nothing of the code under test)"""
    perm = np.random.default_rng(1000 + k).permutation(case.B)
    code = (ost & np.uint64(0xff))[perm]
    good = good_strings(ost, omsk)[perm]
    front = [int(np.flatnonzero(m)[0]) for m in (good, code == 1, code == 3) if m.any()]
    order = front + [i for i in range(case.B) if i not in front]
    return perm[order][:n].astype(np.int64)


def good_strings(ost, omsk):
    """status 0, an accepted state, something revealed (the lever definitions of the chunked row accept nothing: status 0 and something revealed there)"""
    code = ost & np.uint64(0xff)
    reveals = (code == 0) & omsk.reshape(len(ost), -1).any(axis=1)
    accepted = reveals & (((ost >> np.uint64(8)) & np.uint64(0xffffffff)) != 0)
    return accepted if accepted.any() else reveals


def handover_selection(B1):
    """call 2 of the scratch handover: the batch without its first string, in reversed order (B2 = B1 - 1 <= B1: no reserve() regrows the scratch)"""
    return np.arange(B1, dtype=np.int64)[::-1][:max(1, B1 - 1)].copy()


def decoy_bites(ost, omsk):
    """the share of strings b whose status word or masked rows differ from those of string B - 1 - b"""
    differs = (ost != ost[::-1]) | (omsk != omsk[::-1]).reshape(len(ost), -1).any(axis=1)
    return float(differs.mean())


# ---- the match cases (fused narrow / L2 / HALF table, via rows; ragged; selected over both sources) --------------------------------------------------
MATCH_VARIANTS = [("narrow", 0x80000), ("global", 0x40000), ("half", 0x400000), ("via_rows", 1 << 32)]      # (name, HRX_DEBUG_FLAGS) as tests/test_match_gpu.py VARIANTS
MATCH_SPANS = 8


def match_case(D=2):
    """B = 129 strings of 1 .. 3 small defs: tests/test_match_gpu.py test_variant_matrix's generator at its smallest batch with more than one workgroup"""
    return fd.make_case({1: 14, 2: 4, 3: 19}[D], fd.Shape(D, D, "small", "any"))
