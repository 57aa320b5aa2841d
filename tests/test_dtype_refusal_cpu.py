"""A dtype code that is neither MRMT3_F32 (0) nor MRMT3_BF16 (1) is refused with MRMT3_ERR_INVALID_ARG by every entry
point that dispatches on one through mr_dtype (csrc/common.h), before anything is launched or written, whether or not the
operand the code describes is null; the message names the entry point and the argument.  Before, each entry point's ladder
fell through to one of its kernels, which then read the caller's memory as the wrong type.

No GPU is needed: with the code 7 the call returns before its launch.  With the codes 0 and 1 and otherwise valid small
sizes the call gets past that check; it may fail later for lack of a device, so only the message is looked at.  On a machine
that has a GPU those calls do launch, so the operands are then disjoint pieces of a zeroed device buffer, large enough for
every size below (zeros are valid targets, ids and logits)."""
import ctypes

import pytest
import torch

from mrmt3 import lib

INVALID_ARG = 1
SLOT, SLOTS = 64 * 1024, 64


@pytest.fixture(scope="module")
def P():
    """P(k): the address of the k-th 64 KiB piece of a zeroed buffer (device memory where there is a device)"""
    if torch.cuda.is_available():
        buf = torch.zeros(SLOT * SLOTS, dtype=torch.uint8, device="cuda:0")
        base = buf.data_ptr()
    else:
        buf = (ctypes.c_uint8 * (SLOT * SLOTS + 256))()
        base = (ctypes.addressof(buf) + 255) & ~255
    yield lambda k: ctypes.c_void_p(base + k * SLOT)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del buf


def _norm_fwd(so, P, c, null=False):
    return so.mrmt3_add_rmsnorm_fwd(P(0), None if null else P(1), c["y_dtype"], P(2), 1e-6, P(3), P(4), c["xn_dtype"], P(5), 1, 256,
                                    0.0, 0, None, 0, 0, 0, None)


def _norm_bwd(so, P, c, null=False):
    return so.mrmt3_add_rmsnorm_bwd(P(0), c["dxn_dtype"], None if null else P(1), c["dres_dtype"], P(2), P(3), P(4), P(5),
                                    c["dx1_dtype"], P(6), None, 1, 512, 0.0, 0, None, 0, 0, 0, None, 0, None)


def _geglu_fwd(so, P, c, null=False):
    return so.mrmt3_geglu_fwd(P(0), P(1), 1, 8, c["dtype"], 0.0, 0, None, 0, None)


def _geglu_bwd(so, P, c, null=False):
    return so.mrmt3_geglu_bwd(P(0), P(1), P(2), 1, 8, c["dtype"], 0.0, 0, None, 0, None)


def _addpos(so, P, c, null=False):
    return so.mrmt3_addpos_fwd(P(0), c["src_dtype"], P(1), P(2), 1, 1, 4, 0, 0.0, 0, None, 0, None)


def _dropmask_cast(so, P, c, null=False):
    return so.mrmt3_dropmask_cast(P(0), P(1), c["out_dtype"], 4, 0.0, 0, None, 0, None)


def _ce(so, P, c, null=False):
    return so.mrmt3_ce_fwd_bwd(P(0), P(1), P(2), P(3), None if null else P(4), c["dl_dtype"], 1, 512, 0, 0, 0, 1.0, None)


def _ce_reg(so, P, c, null=False):
    return so.mrmt3_ce_fwd_bwd_reg(P(0), P(1), P(2), 0.1, 1e-4, P(3), None if null else P(4), c["dl_dtype"], 1, 512, 0, 0, 0, 1.0,
                                   None)


def _cast(so, P, c, null=False):
    return so.mrmt3_cast(P(0), c["in_dtype"], P(1), c["out_dtype"], 4, None)


def _transpose(so, P, c, null=False):
    return so.mrmt3_transpose(P(0), c["in_dtype"], P(1), c["out_dtype"], 2, 2, None)


def _lmhead_ce(so, P, c, null=False):
    return so.mrmt3_lmhead_ce_fwd_bwd(P(0), 64, P(40), 64, P(1), P(2), P(3), None if null else P(4), c["dl_dtype"], 1, 512, 64, 0, 0,
                                      0, 1.0, P(5), 2048, 1024, None)


def _lmhead_ce_reg(so, P, c, null=False):
    return so.mrmt3_lmhead_ce_fwd_bwd_reg(P(0), 64, P(40), 64, P(1), P(2), 0.1, 1e-4, P(3), None if null else P(4), c["dl_dtype"],
                                          1, 512, 64, 0, 0, 0, 1.0, P(5), 2048, 1024, None)


def _lmhead_logprob(so, P, c, null=False):
    return so.mrmt3_lmhead_logprob(P(0), 64, P(40), 64, P(1), P(2), 1, 512, 64, c["dtype"], P(5), 2048, 1024, None)


# the prefix of the entry point's error texts, its dtype arguments, the call, whether an operand a code describes may be null
ENTRIES = [
    ("add_rmsnorm_fwd", ("y_dtype", "xn_dtype"), _norm_fwd, True),
    ("add_rmsnorm_bwd", ("dxn_dtype", "dres_dtype", "dx1_dtype"), _norm_bwd, True),
    ("geglu_fwd", ("dtype",), _geglu_fwd, False),
    ("geglu_bwd", ("dtype",), _geglu_bwd, False),
    ("addpos_fwd", ("src_dtype",), _addpos, False),
    ("dropmask_cast", ("out_dtype",), _dropmask_cast, False),
    ("ce_fwd_bwd", ("dl_dtype",), _ce, True),
    ("ce_fwd_bwd_reg", ("dl_dtype",), _ce_reg, True),
    ("cast", ("in_dtype", "out_dtype"), _cast, False),
    ("transpose", ("in_dtype", "out_dtype"), _transpose, False),
    ("lmhead_ce", ("dl_dtype",), _lmhead_ce, True),
    ("lmhead_ce_reg", ("dl_dtype",), _lmhead_ce_reg, True),
    ("lmhead_logprob", ("dtype",), _lmhead_logprob, False),
]
ARGS = [(who, args, call, nullable, arg) for who, args, call, nullable in ENTRIES for arg in args]


@pytest.mark.parametrize("who,args,call,nullable,arg", ARGS, ids=["%s-%s" % (a[0], a[4]) for a in ARGS])
def test_an_unknown_dtype_code_is_refused_by_name(P, who, args, call, nullable, arg):
    so = lib.load()
    codes = {a: (7 if a == arg else 0) for a in args}
    for null in ((False, True) if nullable else (False,)):
        assert call(so, P, codes, null) == INVALID_ARG
        err = so.mrmt3_last_error()
        assert err.startswith((who + ": " + arg + " = 7 is neither MRMT3_F32 nor MRMT3_BF16").encode()), err


@pytest.mark.parametrize("who,args,call,nullable,arg", ARGS, ids=["%s-%s" % (a[0], a[4]) for a in ARGS])
def test_the_two_known_codes_pass_the_dtype_check(P, who, args, call, nullable, arg):
    so = lib.load()
    for code in (0, 1):
        rc = call(so, P, {a: (code if a == arg else 0) for a in args})
        assert rc == 0 or b"is neither MRMT3_F32 nor MRMT3_BF16" not in so.mrmt3_last_error(), so.mrmt3_last_error()
