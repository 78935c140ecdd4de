"""False accepts of VERIFY on the device (verify_rows_kernel<DT, T, REC> of csrc/hrx_kernel_verify.hip), in every one of its fifteen instantiations and on every
branch it takes at run time on the input layout and the row stripes.  tests/test_verify_gpu.py shows that clean rows pass in every form; here rows that must NOT
pass are judged in every form, and cells that must not be judged at all are poisoned.

  matrix             the catalogue of tests/verify_cases.py (one cell changed per string, at the borders of every tile size, of n and of M, values outside the tables
                     included) x eight def sets — one per DT, 304 states, two substring ids — x string-major tight / pitched, position-major from both input
                     layouts, planes / row stripes from both.  The rows are witnessed on the device and changed there, addressed as the form lays them out; copied
                     back they must be the rows tests/test_verify_cases_cpu.py changed on the host, the words the host twin's, the bits the torch checker's, and
                     every entry must do what the catalogue's a-priori table says.  Before the mutations every never-judged cell — the tail rows of the last quad
                     and octet, the rows between M and the pitch, the input bytes from n on — is filled with values no table holds: no word may move.
  small circuits     M = 1 .. 33 x one to five defs x every form, 70 strings of n = 0, 1, M - 1, M: clean, poisoned, and with the state and the masked cell of
                     row M - 1 changed
  second block       65536 + 300 strings x 19 rows in planes and in the two row stripes of one def (3 and 2 quads): one record per plane / stripe, one masked
                     cell and one input byte of strings of the second block
  wrong lengths      verify called with n - 1 and n + 1 on clean rows

The out-of-range kinds (state_out, sid_out, fl7) rest on the clamps of verify_def_look; tests/host_cpp/test_verify_host.cpp runs them under the address sanitizer
on the host, with the image a heap block of its exact size, in every instantiation of the tile loop.  Every verdict buffer lies between two poisoned 4-KiB guards."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import carry_defs as cd
import fr_cases as fc
import halo2_regex_amd as hra
import verify_cases as vc
from mock_prover import FAIL_ACCEPT
from test_verify_cases_cpu import ALL_BUT_ENABLE, LOW, check_classes, defs_of_text, expected, torch_words
from test_verify_gpu import ALL_FORMS, DEV, Rows

pytestmark = pytest.mark.gpu
POISON = (vc.POISON_REC, vc.POISON_MSK, vc.POISON_CHAR)


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: string %d: %s, expected %s (%d strings differ)" % (what, bad[0], hra.explain_verdict(got[bad[0]]), hra.explain_verdict(want[bad[0]]), len(bad))


def same_rows(rows, rec_want, msk_want, what):
    rec, msk = rows.host_rows()
    assert np.array_equal(rec, rec_want) and np.array_equal(msk, msk_want), "%s: the rows on the device are not the expected ones" % what


def poison_and_count(rows):
    """every never-judged cell of this form poisoned; the number of cells is what the form's shape gives"""
    B, M, D, form = rows.B, rows.M, rows.D, rows.form
    count = rows.poison_unjudged(*POISON)
    if form.startswith("sm"):
        rp, mp = hra.recommended_pitches(M)[:2] if "pitched" in form else (M, M)
        assert count["rec"] == B * (rp - M) * D and count["msk"] == B * (mp - M) and ("pitched" not in form or (rp > M and mp > M))
    else:
        assert count["rec"] == B * ((M + 3) // 4 * 4 - M) * D and count["msk"] == B * ((M + 7) // 8 * 8 - M)
    assert count["chr"] == int((rows.stride - rows.lens.astype(np.int64)).sum())
    return count


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("name", list(vc.SETS))
def test_tamper_matrix_every_kernel(name, form):
    e = expected(name)
    cat = e.cat
    what = "%s %s" % (name, form)
    cfg = hra.RegexVerifyConfig.configure(cat.M, defs_of_text(cat.defs_t), device=0)
    rows = Rows(cfg, form, cat.chars, cat.lens)
    assert (rows.planes is None) or len(rows.planes) == (2 if cat.D == 1 else cat.D)
    assert (rows.st.cpu().numpy() & 0xff == 0).all()
    same_rows(rows, e.rec, e.msk, what + " witness")
    same_words(rows.verify(), e.clean, what + " clean")
    # never-judged cells
    count = poison_and_count(rows)
    assert count["chr"] > 0 and (form == "sm" or (count["rec"] > 0 and count["msk"] > 0))
    same_words(rows.verify(), e.clean, what + " poisoned")
    same_rows(rows, e.rec, e.msk, what + " poisoned")
    # the catalogue
    rows.apply(cat)
    same_rows(rows, e.rec_mut, e.msk_mut, what + " mutated")
    live = np.arange(cat.stride)[None, :] < cat.lens[:, None]
    assert np.array_equal(np.where(live, rows.host_chars(), 0), np.where(live, e.chars_mut, 0)), what + ": the input on the device is not the expected one"
    got = rows.verify()
    same_words(got, e.want, what + " mutated")
    assert np.array_equal((got & LOW).astype(np.int64), e.bits), what + ": bits differ from the torch checker's"
    seen = check_classes(cat, e.cls, got, e.clean, tag=form + " ")
    assert seen == ALL_BUT_ENABLE, "checks never seen: %s" % hra.explain_verdict(ALL_BUT_ENABLE & ~seen)


SMALL_M = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
REFUSED = {}          # (D, M, form) -> error code: what the witness entry points refuse at these shapes (none)


@pytest.mark.parametrize("D", (1, 2, 3, 4, 5))
def test_small_circuits(D):
    """M below, at and just above every tile size (8, 16, 32 rows), so that a circuit is less than one tile, exactly one, or one and a row; 70 strings: a partial second
    wave.  Device == host twin of the rows copied back == torch bits, clean, with the never-judged cells poisoned (at M = 1 seven of the octet's eight rows), and with the
    state of row M - 1 changed in every string and its masked cell in every second one"""
    defs_t = cd.lever_defs(D)
    refused = {}
    for M in SMALL_M:
        chars, lens = vc.small_batch(D, M)
        B = len(lens)
        cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(defs_t), device=0)
        for form in ALL_FORMS:
            what = "D %d M %d %s" % (D, M, form)
            try:
                rows = Rows(cfg, form, chars, lens)
            except hra.HrxError as err:
                refused[(D, M, form)] = err.code
                continue
            ok = rows.st.cpu().numpy() & 0xff == 0
            assert ok.all(), what
            rec, msk = rows.host_rows()
            clean = rows.verify()
            same_words(clean, cfg.verify_rows_host(chars, lens, rec, msk), what + " clean")
            assert np.array_equal((clean & LOW).astype(np.int64), torch_words(cfg, chars, lens, rec, msk)), what
            assert ((clean & LOW & ~np.uint64(FAIL_ACCEPT)) == 0).all(), what
            poison_and_count(rows)
            same_words(rows.verify(), clean, what + " poisoned")
            b = np.arange(B)
            which, idx = rows.rec_cells(b, np.full(B, M - 1), b % D)
            rows.update(rows.rec_buffers(), which, idx, np.full(B, 0xffffffff), np.ones(B))
            odd = b[1::2]
            rows.update([rows.msk_buffer()], np.zeros(len(odd)), rows.msk_cells(odd, np.full(len(odd), M - 1)), np.full(len(odd), 0xffff), np.full(len(odd), 0x0101))
            rec2, msk2 = rows.host_rows()
            assert (rec2 != rec).sum() == B and (rec2[b, M - 1, b % D] == rec[b, M - 1, b % D] ^ 1).all() and (msk2 != msk).sum() == len(odd), what
            got = rows.verify()
            same_words(got, cfg.verify_rows_host(chars, lens, rec2, msk2), what + " mutated")
            assert np.array_equal((got & LOW).astype(np.int64), torch_words(cfg, chars, lens, rec2, msk2)), what
            assert (got[1::2] != 0).all() and (got[lens >= max(M - 1, 1)] != 0).all(), what      # a masked cell of 0x0101 ^ what it held; the pair (M - 2, M - 1) or the first-state gate
    print("refused by the witness entry points:", refused)
    assert refused == {k: v for k, v in REFUSED.items() if k[0] == D}


def tall_sets():
    return {"one": [fc.sweep_def(fc.BIG_SWEEP_L)], "two": [fc.sweep_def(fc.BIG_SWEEP_L, 0, 6), fc.sweep_def(fc.BIG_SWEEP_L, 6, 9)]}


@pytest.mark.parametrize("name,form", [("one", "planes"), ("one", "planes-in"), ("two", "planes"), ("two", "planes-in")])
def test_second_block_in_planes_and_stripes(name, form):
    """65536 + 300 strings x 19 rows (5 quads, 3 octets): the second block's string count and its offset — (q4 + R - 1) / R slots a string with R = 2 stripes, 3 and 2
    quads — enter every index of the second block.  Clean: the host twin's words.  Then on string 65536 + 5 one record per stripe (rows 9 and 13: slot 1 of either
    stripe) or per plane, one masked cell (row 17), and with a position-major input its byte 0 (its n is 1) and byte 17 of string 65536 + 1 (n = 19; chunk 1 of the
    block): exactly those strings change, to the host twin's words"""
    chars, lens = fc.tall_batch()
    B, M = len(lens), 19
    assert B == 65536 + 300 and chars.shape[1] == 32
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(tall_sets()[name]), device=0)
    D = cfg.num_defs
    rows = Rows(cfg, form, chars, lens)
    assert len(rows.planes) == 2
    rec, msk = rows.host_rows()
    clean = rows.verify()
    same_words(clean, cfg.verify_rows_host(chars, lens, rec, msk), name + " " + form + " clean")
    assert ((clean & LOW & ~np.uint64(FAIL_ACCEPT)) == 0).all() and (clean == 0).sum() > 1000
    b, b2 = 65536 + 5, 65536 + 1
    assert lens[b] == 1 and lens[b2] == M
    which, idx = rows.rec_cells([b, b], [9, 13], [0, D - 1])
    assert which.tolist() == [0, 1]
    rows.update(rows.rec_buffers(), which, idx, [0xffffffff] * 2, [1, 1])
    rows.update([rows.msk_buffer()], [0], rows.msk_cells([b], [17]), [0xffff], [0x0101])
    touched = [b]
    chars2 = chars.copy()
    if form.endswith("-in"):
        rows.update([rows.chr_buffer()], [0, 0], rows.chr_cells([b, b2], [0, 17]), [0, 0], [cd.UNDEF] * 2)
        chars2[b, 0] = chars2[b2, 17] = cd.UNDEF
        touched = [b2, b]
        assert np.array_equal(rows.host_chars(), chars2)
    rec2, msk2 = rows.host_rows()
    assert (rec2 != rec).sum() == 2 and rec2[b, 9, 0] == rec[b, 9, 0] ^ 1 and rec2[b, 13, D - 1] == rec[b, 13, D - 1] ^ 1 and (msk2 != msk).sum() == 1 and msk2[b, 17] == msk[b, 17] ^ 0x0101
    got = rows.verify()
    same_words(got, cfg.verify_rows_host(chars2, lens, rec2, msk2), name + " " + form + " mutated")
    assert np.nonzero(got != clean)[0].tolist() == touched
    assert int(got[b]) & hra.VERIFY_MASK and int(got[b]) & hra.VERIFY_PADDING and int(got[b]) >> 32 <= 9, hra.explain_verdict(got[b])
    assert not form.endswith("-in") or (int(got[b]) & hra.VERIFY_TRANSITION and int(got[b]) >> 32 == 0 and int(got[b2]) & hra.VERIFY_TRANSITION and int(got[b2]) >> 32 == 17)


@pytest.mark.parametrize("name", ["one", "three", "five"])
def test_lengths_that_disagree_with_the_rows(name):
    """clean rows of the base strings (n = 64, 101, 139 of M = 139) judged with n - 1 — the row that held the last byte carries a tag, a flag or a state that is neither
    the accepted nor the dummy one, or the row behind it a state that is not the dummy — and with n + 1 where n < M: the input's zero padding has no transition.  Every
    form: the device == the host twin == the torch bits, and no string passes"""
    defs_t = vc.defs_text(name)
    M = vc.M_ROWS
    chars, lens = vc.base_batch(name)
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(defs_t), device=0)
    shorter, longer = (lens - 1).astype(np.uint32), np.where(lens < M, lens + 1, lens).astype(np.uint32)
    assert (lens >= 2).all() and (longer != lens).sum() == len(lens) * 2 // 3
    for form in ALL_FORMS:
        rows = Rows(cfg, form, chars, lens)
        rec, msk = rows.host_rows()
        for wrong in (shorter, longer):
            got = rows.verify(lens=torch.from_numpy(wrong.astype(np.int32)).to(DEV))
            same_words(got, cfg.verify_rows_host(chars, wrong, rec, msk), "%s %s" % (name, form))
            assert np.array_equal((got & LOW).astype(np.int64), torch_words(cfg, chars, wrong, rec, msk)), (name, form)
            assert (got[wrong != lens] != 0).all() and (got >> np.uint64(57) == 0).all(), (name, form)
