"""GPU tests of sla_hip_launch_dec_judge (k_dec_judge; run with -m gpu on an MI355X): the verdict of the indexed window
decode, on crafted tables, against the serial loop of tests/indexmodel.py.  Every table is made on the host -- an image
whose chain headers agree with the rows, clean infos -- and then damaged in exactly the way the case is about; the
outcomes, the emit table after the launch and the sentinels around both are compared with the model's.  Nothing here reads
the reference tree."""
import ctypes as C

import numpy as np
import pytest

import indexmodel as IM

pytestmark = pytest.mark.gpu

OK, BUF, SYNTH, DATA, HEADER_FORMAT, CORRUPT = 0, 4, 8, 9, 10, 11
BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
INFO_DT = np.dtype([("type", "<u4"), ("used_bytes", "<u4"), ("crc", "<u4"), ("overrun", "<u4")])
ITEM_DT = np.dtype([("first", "<u4"), ("nb", "<u4"), ("stop", "<u4"), ("ok_samples", "<u4"), ("outcome", "<u4"), ("emit", "<u4"),
                    ("fill_end", "<u4"), ("reserved", "<u4")])
EMIT_DT = np.dtype([("plane_off", "<u8"), ("channel_stride", "<u8"), ("sample_stride", "<u8"), ("dst", "<u8"), ("done", "<u4"),
                    ("fill_end", "<u4"), ("num_channels", "<u4"), ("mid_side", "<u4"), ("shift", "<u4"), ("bits_per_sample", "<u4")])
NO_EMIT = IM.NO_EMIT
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


class Tables:
    """a pass of `nbs[i]` clean rows per item: the image holds each row's chain header at an odd offset, every info says
    "decoded to the byte", every item has an emit entry and outcome slot i"""

    def __init__(self, nbs, seed=1, stops=None):
        rng = np.random.default_rng(seed)
        total = sum(nbs)
        self.blocks = np.zeros(total, BLOCK_DT)
        self.info = np.zeros(total, INFO_DT)
        self.items = np.zeros(len(nbs), ITEM_DT)
        self.emit = np.zeros(len(nbs), EMIT_DT)
        img = bytearray()
        k = 0
        for i, nb in enumerate(nbs):
            self.items[i] = (k, nb, stops[i] if stops else OK, 1000 + i, i, i, 77 + i, 0)
            self.emit[i] = (64 * i, 4096, 1, 0x1000 * (i + 1), 1000 + i, 2000 + i, 2, i & 1, 16, 16)
            for _ in range(nb):
                blen = int(rng.integers(11, 40)) | 1                     # odd lengths: every alignment of a header is met
                n = int(rng.integers(1, 16385))
                crc = int(rng.integers(0, 65536))
                self.blocks[k] = (len(img), blen, 7 * k, n, 0)
                self.info[k] = (int(rng.integers(0, 3)), blen, crc, 0)
                img += b"\xff\xff" + (blen - 6).to_bytes(4, "big") + crc.to_bytes(2, "big") + n.to_bytes(2, "big") + bytes(rng.integers(0, 256, blen - 10, dtype=np.uint8))
                k += 1
        self.image = np.frombuffer(bytes(img) + b"\x00" * 3, np.uint8).copy()
        self.image_bytes = len(img)

    def row(self, item, r):
        return int(self.items[item]["first"]) + r

    def model(self, crc_check, lms_ok, num_outcomes=None, num_emit=None):
        emit = [[int(e["done"]), int(e["fill_end"])] for e in self.emit[:len(self.emit) if num_emit is None else num_emit]]
        rows = [(int(b["byte_off"]), int(b["byte_len"]), int(b["smp_off"]), int(b["num_samples"])) for b in self.blocks]
        infos = [tuple(int(v) for v in i) for i in self.info]
        items = [tuple(int(it[f]) for f in ("first", "nb", "stop", "ok_samples", "outcome", "emit", "fill_end")) for it in self.items]
        out = IM.judge(self.image[:self.image_bytes], rows, infos, items, crc_check, lms_ok, emit,
                       len(self.items) if num_outcomes is None else num_outcomes)
        return out, emit


def launch(hip, t, crc_check=1, lms_ok=1, num_outcomes=None, num_emit=None):
    """-> ({outcome slot: (result, samples)} of the slots that changed, the emit table afterwards), checked against the model"""
    import torch
    L = hip.lib()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).cuda()
    d_img, d_blocks, d_info, d_items, d_emit = up(t.image), up(t.blocks), up(t.info), up(t.items), up(t.emit)
    slots = len(t.items) + 3
    d_out = torch.full((slots, 2), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_judge(C.c_void_p(d_img.data_ptr()), t.image_bytes, C.c_void_p(d_blocks.data_ptr()), C.c_void_p(d_info.data_ptr()),
                                    len(t.blocks), C.c_void_p(d_items.data_ptr()), len(t.items), crc_check, lms_ok,
                                    C.c_void_p(d_emit.data_ptr()), len(t.emit) if num_emit is None else num_emit,
                                    C.c_void_p(d_out.data_ptr()), len(t.items) if num_outcomes is None else num_outcomes, None)
    assert rc == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    got = {i: (int(out[i, 0]), int(out[i, 1])) for i in range(slots) if (out[i] != SENTINEL).any()}
    emit = d_emit.cpu().numpy()[:t.emit.nbytes].view(EMIT_DT) if len(t.emit) else t.emit
    # the inputs are only read
    assert np.array_equal(d_blocks.cpu().numpy()[:t.blocks.nbytes], t.blocks.view(np.uint8).reshape(-1))
    assert np.array_equal(d_info.cpu().numpy()[:t.info.nbytes], t.info.view(np.uint8).reshape(-1))
    want, want_emit = t.model(crc_check, lms_ok, num_outcomes, num_emit)
    assert got == want
    # of the emit table only done / fill_end of failed items moved
    ref = t.emit.copy()
    for e, (done, fill_end) in enumerate(want_emit):
        ref[e]["done"], ref[e]["fill_end"] = done, fill_end
    assert emit.tobytes() == ref.tobytes()
    return got, emit


def fail(t, item, r, how):
    """damage row r of `item` so that exactly rule `how` applies"""
    k = t.row(item, r)
    off = int(t.blocks[k]["byte_off"])
    if how == "sync":
        t.image[off + 1] = 0xFE
    elif how == "size":
        t.image[off + 5] ^= 0x02
    elif how == "count":
        t.image[off + 9] ^= 0x01
    elif how == "crc":
        t.info[k]["crc"] ^= 0x8000
    elif how == "type":
        t.info[k]["type"] = 3
    elif how == "lms":
        t.info[k]["type"] = 0
    elif how == "overrun":
        t.info[k]["overrun"] = 1
    elif how == "used":
        t.info[k]["used_bytes"] -= 1
    else:
        raise ValueError(how)


@pytest.mark.parametrize("nb", [0, 1, 63, 64, 65, 129])
def test_clean_items_of_every_row_count_and_one_failing_row_at_every_position(hip, nb):
    t = Tables([nb], seed=nb)
    got, emit = launch(hip, t)
    assert got == {0: (OK, 1000)} and emit.tobytes() == t.emit.tobytes()         # clean: the emit entry bit for bit as it was
    for r in sorted({0, 62, 63, 64, nb - 1}):
        if not 0 <= r < nb:
            continue
        t = Tables([nb], seed=nb)
        fail(t, 0, r, "type")
        got, emit = launch(hip, t)
        assert got == {0: (HEADER_FORMAT, 0)}, r
        assert (int(emit[0]["done"]), int(emit[0]["fill_end"])) == (0, 77)


@pytest.mark.parametrize("first,second", [(("type", HEADER_FORMAT), ("overrun", CORRUPT)), (("used", CORRUPT), ("type", HEADER_FORMAT))])
@pytest.mark.parametrize("rows", [(3, 4), (10, 100), (63, 64), (0, 128), (64, 65), (5, 69)])
def test_the_earlier_of_two_failing_rows_wins(hip, first, second, rows):
    t = Tables([129], seed=5)
    fail(t, 0, rows[0], first[0])
    fail(t, 0, rows[1], second[0])
    got, _ = launch(hip, t)
    assert got == {0: (first[1], 0)}


@pytest.mark.parametrize("how,code", [("sync", CORRUPT), ("size", CORRUPT), ("count", CORRUPT), ("crc", CORRUPT), ("type", HEADER_FORMAT),
                                      ("overrun", CORRUPT), ("used", CORRUPT)])
def test_each_row_rule_alone(hip, how, code):
    t = Tables([7, 70], seed=11)
    fail(t, 1, 66, how)
    got, emit = launch(hip, t)
    assert got == {0: (OK, 1000), 1: (code, 0)}
    assert (int(emit[0]["done"]), int(emit[0]["fill_end"])) == (1000, 2000) and (int(emit[1]["done"]), int(emit[1]["fill_end"])) == (0, 78)


def test_lms_rule_and_what_is_no_failure(hip):
    t = Tables([70], seed=12)
    t.info["type"][:] = 1
    t.info["type"][::2] = 2
    assert launch(hip, t, lms_ok=0)[0] == {0: (OK, 1000)}            # silent and raw rows need no LMS stage
    t.info["type"][65] = 0
    assert launch(hip, t, lms_ok=0)[0] == {0: (SYNTH, 0)}
    assert launch(hip, t, lms_ok=1)[0] == {0: (OK, 1000)}


def test_rule_order_within_a_row_and_the_crc_switch(hip):
    t = Tables([66], seed=13)
    fail(t, 0, 65, "overrun"); fail(t, 0, 65, "crc"); fail(t, 0, 65, "type")
    assert launch(hip, t, crc_check=1)[0] == {0: (CORRUPT, 0)}       # the CRC speaks before the type
    assert launch(hip, t, crc_check=0)[0] == {0: (HEADER_FORMAT, 0)}  # ... and not at all when it is off
    t = Tables([66], seed=13)
    fail(t, 0, 2, "crc")
    assert launch(hip, t, crc_check=0)[0] == {0: (OK, 1000)}
    t = Tables([66], seed=13)
    fail(t, 0, 2, "type"); fail(t, 0, 2, "count")
    assert launch(hip, t, crc_check=0)[0] == {0: (CORRUPT, 0)}       # a stale index speaks first
    t = Tables([66], seed=13)
    fail(t, 0, 2, "lms"); fail(t, 0, 2, "overrun")
    assert launch(hip, t, lms_ok=0)[0] == {0: (SYNTH, 0)}


def test_stop_codes_five_items_and_an_item_without_an_emit_entry(hip):
    t = Tables([3, 0, 65, 0, 129], seed=14, stops=[OK, DATA, BUF, OK, OK])
    t.items["emit"][2] = NO_EMIT
    t.items["emit"][1] = 1
    fail(t, 4, 128, "used")
    got, emit = launch(hip, t)                                        # five items: two workgroups, the second of one wave
    assert got == {0: (OK, 1000), 1: (DATA, 0), 2: (BUF, 0), 3: (OK, 1003), 4: (CORRUPT, 0)}
    assert [int(e["done"]) for e in emit] == [1000, 0, 1002, 1003, 0]
    assert [int(e["fill_end"]) for e in emit] == [2000, 78, 2002, 2003, 81]
    # a row failure outranks the stop code
    fail(t, 2, 64, "type")
    assert launch(hip, t)[0][2] == (HEADER_FORMAT, 0)


def test_positions_outside_the_tables_are_not_touched(hip):
    t = Tables([5, 5, 5], seed=15)
    t.items["nb"][1] = 11                                             # rows past the table: judged NG, nothing of them read
    t.items["outcome"][2] = 2
    fail(t, 2, 0, "type")
    got, emit = launch(hip, t, num_outcomes=2, num_emit=2)            # item 2's outcome and emit entry lie outside
    assert got == {0: (OK, 1000), 1: (1, 0)}
    assert int(emit[2]["done"]) == 1002
    t = Tables([2], seed=16)
    t.blocks["byte_off"][1] = t.image_bytes - 9                       # a chain header that does not lie inside the image
    assert launch(hip, t)[0] == {0: (CORRUPT, 0)}
