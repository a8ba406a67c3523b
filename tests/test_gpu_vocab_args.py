"""GPU tests of what mrg_vocab_encode, mrg_vocab_decode, mrg_vocab_term_counts and mrg_vocab_postings answer
to a call with exactly one invalid argument: the status code and the whole mrg_last_error() text, one case per
argument check of the host layer.  The entry points are called through ctypes directly, so that a null
vocabulary, a null offsets array or n_docs = 0xFFFFFFFF can be passed at all.  The expected strings are written
out here, not taken from the library.  Every case is refused on the host, or by the kernels' own bounds-checked
validation of the ids.  A last test pins which diagnostics a call clears and which it leaves
(mrg_encode_info, mrg_decode_info, mrg_postings_info).  A null context is covered by the *_cpu.py files."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNK = 0xFFFFFFFF
DOCS = [b"a b c a", b"b c"]          # as ids: 0 1 2 0 | 1 2
IDS = [0, 1, 2, 0, 1, 2]
TOK_OFF = [0, 4, 6]
TERMS, COUNTS, ROW_OFF = [0, 1, 2, 1, 2], [2, 1, 1, 1, 1], [0, 3, 5]
DOWN = [0, 5, 3]                     # decreasing at index 1
NO_DOCS = "null offsets (h_doc_off and h_tok_off need n_docs + 1 entries)"
NO_TOKS = "null offsets (h_tok_off and h_out_off need n_docs + 1 entries)"
NO_ROWS = "null offsets (h_tok_off and h_row_off need n_docs + 1 entries)"
OTHER_DEVICE = "the vocabulary lives on device 1, the context on device 0"


def u64(xs):
    return (C.c_uint64 * len(xs))(*xs)


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vocab(ctx):
    v = ctx.vocab_from_text(b"a 3\nb 2\nc 1\n")
    yield v
    v.close()


class Dev:
    """the device buffers of every call: the text, the ids, the CSR, and destinations with room to spare"""

    def __init__(self):
        import torch
        from gpu_util import to_device
        from terms_util import ids_to_device
        self.text, self.doc_off = to_device(DOCS)
        self.ids = ids_to_device(IDS)
        self.terms, self.counts = ids_to_device(TERMS), ids_to_device(COUNTS)
        self.out = torch.zeros((4, 64), dtype=torch.int32, device="cuda:0")        # four 256-byte destinations
        self.post_off = torch.zeros((8,), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()                             # the context runs on a stream of its own

    def o(self, i):
        return self.out[i].data_ptr()


@pytest.fixture(scope="module")
def dev():
    return Dev()


def call(name, *args):
    """(status, mrg_last_error text) of one entry point"""
    from mapreduce_rust_amd import native
    L = native.load()
    rc = getattr(L, name)(*args)
    return rc, (L.mrg_last_error().decode() if rc else "")


def refused(name, args, cases):
    """`args` is a good call (name: position); every case replaces some arguments and names the message"""
    from mapreduce_rust_amd import native
    names = list(args)
    rc, msg = call(name, *args.values())
    assert rc == native.OK, msg
    for what, change, text in cases:
        a = dict(args)
        assert set(change) <= set(names), what
        a.update(change)
        rc, msg = call(name, *a.values())
        assert (rc, msg) == (native.EINVAL, text), (name, what, rc, msg)
    rc, msg = call(name, *args.values())                     # and the good call still is one
    assert rc == native.OK, msg


def test_encode(ctx, vocab, dev):
    tok = u64([0, 0, 0])
    good = dict(c=ctx.h, v=vocab.h, d_bytes=dev.text.data_ptr(), h_doc_off=u64(dev.doc_off), n_docs=2, d_ids=None,
                cap_ids=0, h_tok_off=tok)
    rc, msg = call("mrg_vocab_encode", *good.values())
    assert rc == 0 and list(tok) == TOK_OFF, msg
    n = tok[2]
    refused("mrg_vocab_encode", good, [
        ("null vocabulary", dict(v=None), "null vocabulary"),
        ("null h_doc_off", dict(h_doc_off=None), NO_DOCS),
        ("null h_tok_off", dict(h_tok_off=None), NO_DOCS),
        ("decreasing", dict(h_doc_off=u64(DOWN)), "document offsets must be non-decreasing"),
        ("n_docs", dict(n_docs=0xFFFFFFFF), "n_docs out of range"),
        ("misaligned d_bytes", dict(d_bytes=dev.text.data_ptr() + 1), "input buffer must be 16-byte aligned"),
        ("null d_bytes", dict(d_bytes=None), "null input"),
        ("cap", dict(d_ids=dev.o(0), cap_ids=n - 1), "destination too small (%d ids < %d tokens)" % (n - 1, n)),
    ])
    good.update(d_ids=dev.o(0), cap_ids=n)
    assert call("mrg_vocab_encode", *good.values())[0] == 0
    assert dev.out[0][:n].cpu().tolist() == IDS


def test_decode(ctx, vocab, dev):
    out = u64([0, 0, 0])
    good = dict(c=ctx.h, v=vocab.h, d_ids=dev.ids.data_ptr(), h_tok_off=u64(TOK_OFF), n_docs=2, h_unk=None, unk_len=0,
                d_out=None, cap=0, h_out_off=out)
    rc, msg = call("mrg_vocab_decode", *good.values())
    assert rc == 0 and list(out) == [0, 8, 12], msg
    n = out[2]
    refused("mrg_vocab_decode", good, [
        ("null vocabulary", dict(v=None), "null vocabulary"),
        ("null h_tok_off", dict(h_tok_off=None), NO_TOKS),
        ("null h_out_off", dict(h_out_off=None), NO_TOKS),
        ("decreasing", dict(h_tok_off=u64(DOWN)), "token offsets must be non-decreasing"),
        ("n_docs", dict(n_docs=0xFFFFFFFF), "n_docs out of range"),
        ("misaligned d_ids", dict(d_ids=dev.ids.data_ptr() + 2), "the ids must be 4-byte aligned"),
        ("null d_ids", dict(d_ids=None), "null ids"),
        ("unk_len 256", dict(h_unk=bytes(256), unk_len=256), "unk_len 256: at most 255 bytes"),
        ("null h_unk", dict(unk_len=3), "null h_unk with unk_len 3"),
        ("cap", dict(d_out=dev.o(0), cap=n - 1), "destination too small (%d bytes < %d bytes of text)" % (n - 1, n)),
    ])
    good.update(d_out=dev.o(0), cap=n)
    assert call("mrg_vocab_decode", *good.values())[0] == 0
    assert bytes(dev.out[0].cpu().numpy().view(np.uint8)[:n]) == b"a b c a\nb c\n"


def test_term_counts(ctx, vocab, dev):
    row = u64([0, 0, 0])
    good = dict(c=ctx.h, v=vocab.h, d_ids=dev.ids.data_ptr(), h_tok_off=u64(TOK_OFF), n_docs=2, d_terms=None,
                d_counts=None, cap=0, h_row_off=row, h_unk=None)
    rc, msg = call("mrg_vocab_term_counts", *good.values())
    assert rc == 0 and list(row) == ROW_OFF, msg
    n = row[2]
    both = "d_terms and d_counts must both be given, or both be NULL (sizes only)"
    refused("mrg_vocab_term_counts", good, [
        ("null vocabulary", dict(v=None), "null vocabulary"),
        ("null h_tok_off", dict(h_tok_off=None), NO_ROWS),
        ("null h_row_off", dict(h_row_off=None), NO_ROWS),
        ("decreasing", dict(h_tok_off=u64(DOWN)), "token offsets must be non-decreasing"),
        ("n_docs", dict(n_docs=0xFFFFFFFF), "n_docs out of range"),
        ("misaligned d_ids", dict(d_ids=dev.ids.data_ptr() + 2), "the ids must be 4-byte aligned"),
        ("null d_ids", dict(d_ids=None), "null ids"),
        ("d_terms alone", dict(d_terms=dev.o(0), cap=n), both),
        ("d_counts alone", dict(d_counts=dev.o(1), cap=n), both),
        ("misaligned d_terms", dict(d_terms=dev.o(0) + 2, d_counts=dev.o(1), cap=n),
         "d_terms and d_counts must be 4-byte aligned"),
        ("cap", dict(d_terms=dev.o(0), d_counts=dev.o(1), cap=n - 1),
         "destination too small (%d entries < %d row entries)" % (n - 1, n)),
    ])
    good.update(d_terms=dev.o(0), d_counts=dev.o(1), cap=n)
    assert call("mrg_vocab_term_counts", *good.values())[0] == 0
    assert dev.out[0][:n].cpu().tolist() == TERMS and dev.out[1][:n].cpu().tolist() == COUNTS


def test_postings(ctx, vocab, dev):
    e = C.c_uint64(77)
    good = dict(c=ctx.h, v=vocab.h, d_terms=dev.terms.data_ptr(), d_counts=dev.counts.data_ptr(), h_row_off=u64(ROW_OFF),
                n_docs=2, doc_base=0, d_post_off=dev.post_off.data_ptr(), d_docs=None, d_tf=None, cap=0,
                h_entries=C.pointer(e))
    rc, msg = call("mrg_vocab_postings", *good.values())
    assert rc == 0 and e.value == 5, msg
    n = e.value
    full = dict(d_docs=dev.o(0), d_tf=dev.o(1), cap=n)
    refused("mrg_vocab_postings", good, [
        ("null vocabulary", dict(v=None), "null vocabulary"),
        ("null h_row_off", dict(h_row_off=None), "null offsets (h_row_off needs n_docs + 1 entries)"),
        ("decreasing", dict(h_row_off=u64(DOWN)), "row offsets must be non-decreasing (row 1)"),
        ("doc_base", dict(doc_base=0xFFFFFFFF), "doc_base + n_docs = 4294967297: documents are 32 bits"),
        ("null d_post_off", dict(d_post_off=None), "null d_post_off (it receives the vocabulary's words + 1 offsets)"),
        ("d_tf without d_docs", dict(d_tf=dev.o(1), cap=n), "d_tf without d_docs"),
        ("d_tf without d_counts", dict(full, d_counts=None), "d_tf without d_counts"),
        ("misaligned d_terms", dict(d_terms=dev.terms.data_ptr() + 2),
         "d_terms, d_counts, d_docs and d_tf must be 4-byte aligned"),
        ("misaligned d_post_off", dict(d_post_off=dev.post_off.data_ptr() + 4), "d_post_off must be 8-byte aligned"),
        ("cap", dict(full, cap=n - 1), "destination too small (%d entries < %d postings)" % (n - 1, n)),
        ("null d_terms", dict(d_terms=None), "null terms"),
    ])
    good.update(full)
    assert call("mrg_vocab_postings", *good.values())[0] == 0
    assert dev.post_off[:4].cpu().tolist() == [0, 1, 3, 5]
    assert dev.out[0][:n].cpu().tolist() == [0, 0, 1, 0, 1] and dev.out[1][:n].cpu().tolist() == [2, 1, 1, 1, 1]


@pytest.mark.parametrize("at", [0, 3, 5])
def test_an_id_or_term_that_is_no_word_reports_its_index(ctx, vocab, dev, at):
    from mapreduce_rust_amd import native
    from terms_util import ids_to_device
    import torch
    off = u64([0, 0, 0])
    for bad, unk, tail in ((3, b"", "; MRG_ID_UNK needs unk_len > 0"), (3, b"?", ""),
                           (UNK, b"", "; MRG_ID_UNK needs unk_len > 0")):
        ids = list(IDS)
        ids[at] = bad
        t = ids_to_device(ids)
        torch.cuda.synchronize()
        rc, msg = call("mrg_vocab_decode", ctx.h, vocab.h, t.data_ptr(), u64(TOK_OFF), 2, unk or None, len(unk), None, 0, off)
        assert (rc, msg) == (native.EINVAL, "mrg_vocab_decode: the id at index %d is not in the vocabulary (3 words%s)"
                             % (at, tail)), (bad, unk)
        if bad == UNK:
            continue                                         # (term_counts counts ID_UNK apart: no error)
        rc, msg = call("mrg_vocab_term_counts", ctx.h, vocab.h, t.data_ptr(), u64(TOK_OFF), 2, None, None, 0, off, None)
        assert (rc, msg) == (native.EINVAL,
                             "mrg_vocab_term_counts: the id at index %d is not in the vocabulary (3 words)" % at)
    if at < len(TERMS):
        terms = list(TERMS)
        terms[at] = 3
        t = ids_to_device(terms)
        torch.cuda.synchronize()
        rc, msg = call("mrg_vocab_postings", ctx.h, vocab.h, t.data_ptr(), None, u64(ROW_OFF), 2, 0,
                       dev.post_off.data_ptr(), None, None, 0, None)
        assert (rc, msg) == (native.EINVAL,
                             "mrg_vocab_postings: the term at index %d is not in the vocabulary (3 words)" % at)


def test_vocabulary_of_another_device(ctx, dev):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    off = u64([0, 0, 0])
    with M.Context(1) as other:
        with other.vocab_from_text(b"a 3\nb 2\nc 1\n") as v1:
            for name, args in (
                    ("mrg_vocab_encode", (dev.text.data_ptr(), u64(dev.doc_off), 2, None, 0, off)),
                    ("mrg_vocab_decode", (dev.ids.data_ptr(), u64(TOK_OFF), 2, None, 0, None, 0, off)),
                    ("mrg_vocab_term_counts", (dev.ids.data_ptr(), u64(TOK_OFF), 2, None, None, 0, off, None)),
                    ("mrg_vocab_postings", (dev.terms.data_ptr(), None, u64(ROW_OFF), 2, 0, dev.post_off.data_ptr(), None,
                                            None, 0, None))):
                assert call(name, ctx.h, v1.h, *args) == (M.native.EINVAL, OTHER_DEVICE), name


def test_what_a_call_clears_of_its_diagnostics(ctx, dev):
    """encode keeps the time of the last mrg_job_vocab, decode that of the last mrg_vocab_from_text; a
    postings call clears all of its own"""
    import mapreduce_rust_amd as M
    ctx.set_timing(True)
    try:
        with ctx.vocab_from_text(b"a 3\nb 2\nc 1\n") as v:
            assert ctx.decode_info()["ms_from_text"] > 0
            assert ctx.decode(v, dev.ids.data_ptr(), TOK_OFF, dev.o(0), 256) == [0, 8, 12]
            info = ctx.decode_info()
            assert info["ms_from_text"] > 0 and info["ms_count"] > 0 and info["ids"] == 6
            assert ctx.decode(v, dev.ids.data_ptr(), [0, 0, 0]) == [0, 0, 0]          # no ids: the call's own are cleared
            info = ctx.decode_info()
            assert info["ms_from_text"] > 0 and info["ms_count"] == 0 and info["ms_emit"] == 0 and info["ids"] == 0
        ctx.job_begin(M.APP_WC, 1, M.FLAG_NO_COMPAT_DROP_LAST)
        ctx.set_input(dev.text.data_ptr(), dev.doc_off)
        ctx.map()
        with ctx.vocab() as v:
            assert v.words() == [b"a", b"b", b"c"]
            assert ctx.encode_info()["ms_vocab"] > 0
            for _ in range(2):
                assert ctx.encode(v, dev.text.data_ptr(), dev.doc_off, dev.o(0), 64) == TOK_OFF
                info = ctx.encode_info()
                assert info["ms_vocab"] > 0 and info["ms_count"] > 0 and info["tokens"] == 6
            assert ctx.encode(v, dev.text.data_ptr(), [0, 0, 0]) == [0, 0, 0]         # no bytes
            info = ctx.encode_info()
            assert info["ms_vocab"] > 0 and info["ms_count"] == 0 and info["ms_emit"] == 0 and info["tokens"] == 0
            P = (dev.terms.data_ptr(), dev.counts.data_ptr())
            assert ctx.postings(v, *P, ROW_OFF, dev.post_off.data_ptr(), dev.o(0), dev.o(1), 5) == 5
            info = ctx.postings_info()
            ms = [k for k in info if k.startswith("ms_")]
            assert len(ms) == 5 and info["ms_count"] > 0, info
            assert ctx.postings(v, *P, [0, 0, 0], dev.post_off.data_ptr(), dev.o(0), dev.o(1), 5) == 0
            info = ctx.postings_info()
            assert all(info[k] == 0 for k in ms) and info["entries"] == 0 and info["words"] == 3, info
    finally:
        ctx.set_timing(False)
