"""The self-synchronising entropy stage of a3d_jpeg_decode_split (include/a3d.h, "JPEG decode"; csrc/jpeg_decode.hip) as a host model,
on top of jpeg_decode_ref.parse: a unit's stuffed bytes are cut into subsequences, every subsequence is walked speculatively, the exit
state of one becomes the entry state of the next until a round changes nothing, and the fixed point is what one sequential walk of the
unit gives.  tests/test_jpeg_split_host.py holds `decode` to jpeg_decode_ref.coefficients, exactly.

  state       (bit, slot, index) between two syntax elements: `bit` counts the unit's data bits (the 00 behind an FF is no data: a
              position never rests on one), `slot` is the block within the MCU, `index` the next zig-zag coefficient (0: a DC symbol
              is next).  A symbol and its value bits are one element.
  walk        elements are decoded while the position lies in front of the subsequence's end.  An inconsistency (no code in 16 bits, a
              DC symbol above 15, a run or ZRL past coefficient 63) is recorded with the number of blocks begun so far, then the walk
              carries on: it consumes what the law consumes, ends the block and goes to the next slot.
  rounds      round 0 starts subsequence j >= 1 at (its first data bit, slot 0, index 0) and subsequence 0 at the unit's start; in
              every later round a subsequence whose predecessor's exit differs from the entry it last used walks again from there.
              After round r the subsequences 0 .. r hold their true states, so there are at most as many rounds as subsequences.
  positions   an exclusive prefix sum of the begun-block counts gives a subsequence the ordinal of its first block in the unit.
  status      the first inconsistency of the true chain in a block of the unit ends the unit there: BAD_CODE, or SHORT if the
              element ended past the unit's bytes.  Without one the last subsequence walks on (zeros past the bytes) until the unit's
              blocks are done, and a position past the bytes is SHORT.
  write pass  every subsequence walks once more from its true entry and stores AC values at their places and the DC DIFFERENCE at
              coefficient 0; nothing behind the unit's first inconsistency or past its last block is stored.
  DC pass     per unit and component an inclusive sum of the differences in scan order, modulo 2^16, up to the first bad block (that
              block included where its DC symbol was sound: the law keeps what it decoded of it).
"""
from __future__ import annotations

import numpy as np

import jpeg_decode_ref as D
import mjpeg_ref as M

LANES = 1024  # subsequences a unit is cut into at the most: S = max(split_bytes, ceil(unit bytes / LANES))


def _lut(bits, vals):
    """16 leading bits -> length << 8 | symbol, 0 where they start no code."""
    lut = np.zeros(65536, np.int64)
    for (length, code), sym in D._codes(bits, vals).items():
        lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | sym
    return lut.tolist()


class Scan:
    """What every unit of a stream shares: the slots of an MCU, their components and tables, the MCU grid."""

    def __init__(self, p: D.Parsed):
        self.p = p
        self.mx, self.my = -(-p.width // (8 * p.hmax)), -(-p.height // (8 * p.vmax))
        self.total = self.mx * self.my
        self.slots = [(c, j // h, j % h) for c, (h, v, *_r) in enumerate(p.comps) for j in range(h * v)]  # (component, vy, vx)
        self.nslot = len(self.slots)
        luts = {}
        self.tabs = []
        for c in p.comps:
            pair = []
            for bits, vals in (c[3], c[4]):
                key = (tuple(bits), tuple(vals))
                if key not in luts:
                    luts[key] = _lut(bits, vals)
                pair.append(luts[key])
            self.tabs.append(pair)
        self.ri = p.restart if p.restart else self.total
        self.n_units = -(-self.total // self.ri)
        self.units = (list(p.units) + [b""] * self.n_units)[:self.n_units]


class Unit:
    """One unit's bytes: the data bytes (stuffing removed), where each came from, and a 32-bit window at every data bit."""

    def __init__(self, data: bytes):
        a = np.frombuffer(bytes(data), np.uint8)
        self.n = len(a)
        stuffing = np.zeros(self.n, bool)
        stuffing[1:] = (a[1:] == 0) & (a[:-1] == 0xFF)
        self.bytes = a
        self.orig = np.flatnonzero(~stuffing)
        raw = a[~stuffing]
        self.nd = len(raw)
        pad = np.concatenate([raw, np.zeros(8, np.uint8)]).astype(np.uint64)
        k = len(pad) - 4
        w40 = pad[0:k] << np.uint64(32) | pad[1:k + 1] << np.uint64(24) | pad[2:k + 2] << np.uint64(16) | pad[3:k + 3] << np.uint64(8) | pad[4:k + 4]
        at = np.arange(8 * k, dtype=np.int64)
        self.win = ((w40[at >> 3] >> (8 - (at & 7)).astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()

    def first_bit(self, q: int) -> int:
        """The data bit at which stuffed byte q starts (the next data byte's, where q is the 00 behind an FF)."""
        return 8 * int(np.searchsorted(self.orig, q))


def walk(scan: Scan, unit: Unit, state, end, blocks=None, stop_at_bad=False, emit=None):
    """Elements from `state` while the position is in front of data bit `end` (None: no bound).  `blocks` = (ordinal of the first block
    this walk would begin, blocks of the unit): the walk also ends in front of the block with that last ordinal.  -> (exit state,
    blocks begun, blocks begun at the first inconsistency or None, whether that one was a DC symbol).  `emit(kind, begun, index, value)` sees every DC and AC value."""
    bit, slot, idx = state
    win, n_win, nslot = unit.win, len(unit.win), scan.nslot
    begun, bad_at, bad_dc = 0, None, False
    while end is None or bit < end:
        if blocks is not None and idx == 0 and blocks[0] + begun >= blocks[1]:
            break
        w = win[bit] if bit < n_win else 0
        dc, ac = scan.tabs[scan.slots[slot][0]]
        bad = False
        if idx == 0:
            begun += 1
            e = dc[w >> 16]
            length, s = e >> 8, e & 255
            if e == 0:
                bit, bad = bit + 16, True
            elif s > 15:
                bit, bad = bit + length, True
            else:
                v = (w >> (32 - length - s)) & ((1 << s) - 1) if s else 0
                if emit:
                    emit(0, begun, 0, D._extend(v, s))
                bit, idx = bit + length + s, 1
        else:
            e = ac[w >> 16]
            length, r, s = e >> 8, (e >> 4) & 15, e & 15
            if e == 0:
                bit, bad = bit + 16, True
            elif s == 0:
                bit += length
                if r != 15:
                    idx = 64                      # EOB
                elif idx + 16 > 64:
                    bad = True
                else:
                    idx += 16                     # ZRL
            elif idx + r > 63:
                bit, bad = bit + length, True
            else:
                v = (w >> (32 - length - s)) & ((1 << s) - 1)
                if emit:
                    emit(1, begun, idx + r, D._extend(v, s))
                bit, idx = bit + length + s, idx + r + 1
        if bad:
            if bad_at is None:
                bad_at, bad_dc = begun, idx == 0
            idx = 64
            if stop_at_bad:
                slot, idx = (slot + 1) % nslot, 0
                break
        if idx == 64:
            slot, idx = (slot + 1) % nslot, 0
    return (bit, slot, idx), begun, bad_at, bad_dc


def split_size(n_bytes: int, split_bytes: int, lanes: int = LANES) -> int:
    return max(int(split_bytes), -(-n_bytes // lanes), 1)


def synchronise(scan: Scan, unit: Unit, split_bytes: int, lanes: int = LANES):
    """The rounds.  -> (rounds after round 0 that changed something, [per subsequence a dict: first / end (data bits), entry, exit,
    begun, bad_at, ff_last (its last stuffed byte is FF), entry_past_end])."""
    S = split_size(unit.n, split_bytes, lanes)
    n_sub = max(-(-unit.n // S), 1)
    first = [unit.first_bit(j * S) for j in range(n_sub)] + [8 * unit.nd]
    entry = [(first[j], 0, 0) for j in range(n_sub)]
    out = [walk(scan, unit, entry[j], first[j + 1]) for j in range(n_sub)]
    rounds = 0
    for _ in range(1, n_sub):
        exits = [o[0] for o in out]
        changed = False
        for j in range(1, n_sub):
            if exits[j - 1] != entry[j]:
                entry[j], changed = exits[j - 1], True
                out[j] = walk(scan, unit, entry[j], first[j + 1])
        if not changed:
            break
        rounds += 1
    subs = []
    for j in range(n_sub):
        last = min((j + 1) * S, unit.n) - 1
        subs.append(dict(first=first[j], end=first[j + 1], entry=entry[j], exit=out[j][0], begun=out[j][1], bad_at=out[j][2],
                         ff_last=bool(last >= 0 and unit.bytes[last] == 0xFF), entry_past_end=entry[j][0] >= first[j + 1] and unit.n > 0))
    return rounds, subs


def sequential(scan: Scan, unit: Unit, split_bytes: int, lanes: int = LANES):
    """The same subsequence entries from ONE continuing walk of the unit: the state at the first element boundary at or behind every
    subsequence's first bit."""
    S = split_size(unit.n, split_bytes, lanes)
    n_sub = max(-(-unit.n // S), 1)
    first = [unit.first_bit(j * S) for j in range(n_sub)] + [8 * unit.nd]
    state, entries = (0, 0, 0), []
    for j in range(n_sub):
        entries.append(state)
        state = walk(scan, unit, state, first[j + 1])[0]
    return entries


def decode(p: D.Parsed, split_bytes: int, lanes: int = LANES):
    """-> (coefficient planes as jpeg_decode_ref.coefficients gives them, status, rounds (the most of any unit), per unit its subsequences)."""
    scan = Scan(p)
    planes = [np.zeros((scan.my * v, scan.mx * h, 64), np.int64) for h, v, *_ in p.comps]
    status, most, record = D.OK, 0, []
    for k, data in enumerate(scan.units):
        unit = Unit(data)
        m0 = k * scan.ri
        n_blocks = (min(m0 + scan.ri, scan.total) - m0) * scan.nslot
        rounds, subs = synchronise(scan, unit, split_bytes, lanes)
        most = max(most, rounds)
        record.append(subs)
        prefix, ordinal = [], 0
        for s in subs:  # the exclusive prefix sum
            prefix.append(ordinal)
            ordinal += s["begun"]
        bad_lane, limit = None, n_blocks
        for j, s in enumerate(subs):  # the first flagged subsequence of the true chain whose bad block is one of the unit's
            if s["bad_at"] is not None and prefix[j] + s["bad_at"] - 1 < n_blocks:
                bad_lane, limit = j, prefix[j] + s["bad_at"] - 1
                break
        st = D.OK

        def block(ordinal):
            c, vy, vx = scan.slots[ordinal % scan.nslot]
            m = m0 + ordinal // scan.nslot
            h, v = p.comps[c][:2]
            return planes[c][(m // scan.mx) * v + vy, (m % scan.mx) * h + vx]

        for j, s in enumerate(subs):  # the write pass
            if prefix[j] > n_blocks or (bad_lane is not None and j > bad_lane):
                continue
            base = prefix[j]

            def emit(kind, begun, index, value, base=base):
                block(base + begun - 1)[M.ZIGZAG[index]] = value

            is_last = j == len(subs) - 1
            exit_state, _begun, bad_at, bad_dc = walk(scan, unit, s["entry"], None if is_last else s["end"], (base, n_blocks), j == bad_lane, emit)
            if j == bad_lane:
                assert bad_at is not None
                limit += not bad_dc  # the law keeps the bad block's DC value where its DC symbol was sound
                st = max(st, D.SHORT if exit_state[0] > 8 * unit.nd else D.BAD_CODE)
            elif exit_state[2] == 0 and base + _begun >= n_blocks and exit_state[0] > 8 * unit.nd:
                st = max(st, D.SHORT)
        for c, (h, v, *_r) in enumerate(p.comps):  # the DC pass
            pred = 0
            for ordinal in range(limit):
                if scan.slots[ordinal % scan.nslot][0] == c:
                    blk = block(ordinal)
                    pred = D._wrap16(pred + int(blk[0]))
                    blk[0] = pred
        status = max(status, st)
    return planes, status, most, record
