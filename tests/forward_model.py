"""The rules of solo_forward_levels and solo_forward_route (include/solo_mi355x.h) in plain Python integers: the model the host
emulation (tests/test_forward_model.py) and the GPU (tests/test_gpu_forward.py) are compared with, and the scenarios both run.  Nothing
here shares a line with solo_amd/csrc/solo_forward.h: rooms are lists, slots are dicts, the records are built arrival by arrival."""
import numpy as np

NO_LEVEL = 0x7F
TOP = 2 ** 31 - 1                    # the largest packet number a slot's `next` may hold; a forwarded packet number is at most TOP - 1
COUNT_FIELDS = ("forwarded", "rejected", "no_desc", "no_room", "not_selected", "no_slot", "stale", "switches")
ROW_FIELDS = ("min_seq", "max_seq", "dgrams", "sa", "level", "byte", "pad")


# ---- levels -------------------------------------------------------------------------------------------------------------------------------
def key(byte):
    """the order of the bytes of a row: the loudest first, voiced before unvoiced at equal level"""
    return ((byte & 127) << 1) | (0 if byte >> 7 else 1)


def levels(arrivals, level_in, n_rows, default_level):
    """arrivals: rows of (stream, seq, desc, offset, len); level_in: a byte per arrival or None -> a list of n_rows dicts of ROW_FIELDS"""
    rows = [dict(seqs=[], bytes=[]) for _ in range(n_rows)]
    for i, (stream, seq, desc, _, _) in enumerate(np.asarray(arrivals).tolist()):
        if not (0 <= stream < n_rows and desc in (0, 1)):
            continue
        byte = default_level if level_in is None or int(level_in[i]) == 255 else int(level_in[i])
        rows[stream]["seqs"].append(seq)
        if byte != 255:
            rows[stream]["bytes"].append(byte)
    out = []
    for r in rows:
        byte = min(r["bytes"], key=key) if r["bytes"] else NO_LEVEL
        out.append(dict(min_seq=min(r["seqs"]) if r["seqs"] else -1, max_seq=max(r["seqs"]) if r["seqs"] else -1, dgrams=len(r["seqs"]),
                        sa=255 if byte & 128 else 0, level=byte & 127, byte=byte, pad=0))
    return out


def rowinfo_words(rows):
    """the list of levels() as the device holds it: int32 [n_rows, 4]"""
    a = np.zeros((len(rows), 4), np.int64)
    for s, r in enumerate(rows):
        a[s] = (r["min_seq"], r["max_seq"], r["dgrams"], r["sa"] | r["level"] << 8 | r["byte"] << 16 | r["pad"] << 24)
    return a.astype(np.int32)


def rowinfo_of_words(words):
    return [dict(min_seq=int(w[0]), max_seq=int(w[1]), dgrams=int(w[2]), sa=int(w[3]) & 255, level=int(w[3]) >> 8 & 255, byte=int(w[3]) >> 16 & 255,
                 pad=int(w[3]) >> 24 & 255) for w in np.asarray(words).tolist()]


# ---- route --------------------------------------------------------------------------------------------------------------------------------
class Forward:
    """the state of a solo_forward_t: K slots {src, delta, start, next} for each of n_rows rooms"""

    def __init__(self, n_rows, slots):
        self.n_rows, self.K = n_rows, slots
        self.rooms = None
        self.reset()

    def reset(self, rooms=None):
        if rooms is None:
            self.rooms = [[dict(src=-1, delta=0, start=0, next=0) for _ in range(self.K)] for _ in range(self.n_rows)]
        else:
            for r in rooms:
                self.rooms[r] = [dict(src=-1, delta=0, start=0, next=0) for _ in range(self.K)]

    def state(self):
        """int32 [n_rows, 4 K], as solo_forward_get_state gives it"""
        return np.array([[s[f] for s in room for f in ("src", "delta", "start", "next")] for room in self.rooms], np.int64).astype(np.int32)

    def set_state(self, words):
        for r, w in enumerate(np.asarray(words).tolist()):
            self.rooms[r] = [dict(src=w[4 * k], delta=w[4 * k + 1], start=w[4 * k + 2], next=w[4 * k + 3]) for k in range(self.K)]

    def route(self, arrivals, rowinfo, sel, room, n, n_rooms):
        """-> None for a room id outside [-1, n_rooms) (nothing changes); else dict(count, records: every record the call needs, in order,
        per_arrival: the records of each arrival, level_fwd {index: byte}, slot_src [n_rooms][K], forwarded: (room, slot, packet number,
        source) of every forwarded arrival).  cut() applies max_records."""
        K = self.K
        room = [int(v) for v in room[:n]]
        sel = [int(v) for v in sel[:n]]
        if any(r < -1 or r >= n_rooms for r in room):
            return None
        count = dict.fromkeys(COUNT_FIELDS, 0)
        members = [[i for i in range(n) if room[i] == r] for r in range(n_rooms)]
        holds = {}                                                   # row -> (room, slot) after step 1
        for r in range(n_rooms):
            slots = self.rooms[r]
            for s in slots:                                          # step 1: who keeps
                x = s["src"]
                if not (0 <= x < n and room[x] == r and sel[x] != 0):
                    s["src"] = -1
            holders = {s["src"] for s in slots if s["src"] >= 0}
            newcomers = [x for x in members[r] if sel[x] != 0 and x not in holders and rowinfo[x]["dgrams"] > 0]
            for x in newcomers:                                      # increasing row order, lowest free slot first
                free = [k for k in range(K) if slots[k]["src"] < 0]
                if not free:
                    break
                s = slots[free[0]]
                s["src"], s["start"], s["delta"] = x, s["next"], s["next"] - rowinfo[x]["min_seq"]
                count["switches"] += 1
            for k, s in enumerate(slots):
                if s["src"] >= 0:
                    holds[s["src"]] = (r, k)
        records, per_arrival, forwarded = [], [], []
        for stream, seq, desc, offset, length in np.asarray(arrivals).reshape(-1, 5).tolist():     # steps 2 and 3
            mine = []
            if not 0 <= stream < n:
                count["rejected"] += 1
            elif desc not in (0, 1):
                count["no_desc"] += 1
            elif room[stream] < 0:
                count["no_room"] += 1
            elif sel[stream] == 0:
                count["not_selected"] += 1
            elif stream not in holds:
                count["no_slot"] += 1
            else:
                r, k = holds[stream]
                s = self.rooms[r][k]
                q = seq + s["delta"]
                if not s["start"] <= q <= TOP - 1:
                    count["stale"] += 1
                else:
                    count["forwarded"] += 1
                    forwarded.append((r, k, q, stream))
                    mine = [(m * K + k, q, desc, offset, length) for m in members[r] if m != stream]
            per_arrival.append(mine)
            records += mine
        for r in range(n_rooms):                                     # step 4
            for s in self.rooms[r]:
                if s["src"] >= 0:
                    v = rowinfo[s["src"]]["max_seq"] + s["delta"] + 1
                    if s["start"] + 1 <= v <= TOP:
                        s["next"] = max(s["next"], v)
        level_fwd = {}
        for m in range(n):
            if room[m] >= 0:
                for k, s in enumerate(self.rooms[room[m]]):
                    level_fwd[m * K + k] = rowinfo[s["src"]]["byte"] if s["src"] >= 0 else NO_LEVEL
        return dict(count=count, records=records, per_arrival=per_arrival, forwarded=forwarded, level_fwd=level_fwd,
                    slot_src=[[s["src"] for s in self.rooms[r]] for r in range(n_rooms)])


def cut(res, max_records):
    """what a call with this max_records writes: (records int32 [written, 5], the send count)"""
    rec = res["records"]
    w = rec[:max_records]
    return (np.array(w, np.int64).reshape(-1, 5).astype(np.int32),
            dict(records=len(w), records_needed=len(rec), bytes=sum(x[4] for x in w), bytes_needed=sum(x[4] for x in rec), empty=0, refused=0))


def mid_arrival_cut(res):
    """a max_records that ends inside the records of one arrival (the first one with at least two), or None"""
    at = 0
    for mine in res["per_arrival"]:
        if len(mine) >= 2:
            return at + 1 + (len(mine) - 2) // 2
        at += len(mine)
    return None


# ---- the scenarios --------------------------------------------------------------------------------------------------------------------------
A_ROWS, A_ROOMS, A_TICKS = 24, 5, 12
# rows 0 .. 23: rooms of 1, 2, 3, 5 and 12 members and row 23 in none; at tick 6 row 6, which holds a slot of room 3, moves to room 4: rooms of 1,
# 2, 3, 4 and 13.  (24 rows hold the five sizes and the row in no room only in turn.)
A_ROOM_OF = [0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3] + [4] * 12 + [-1]
A_MOVE_TICK, A_MOVER = 6, 6


def scenario_a(seed, K):
    """12 ticks at n = 24: -> a list of dict(arrivals int32 [nd,5], level_in uint8 [nd], default_level, sel uint8 [24], room int32 [24],
    cut: "all" | "mid" | "zero").  Scripted: who is selected when (more than K in room 4, a speaker that stops and returns, a selected row
    without a datagram, the move of a slot holder, a slot handed over near 2^31); random: bursts of 0 .. 3 packets per sender, single
    descriptions, rejected arrivals, desc = -1, levels with and without a byte, late datagrams."""
    rng = np.random.default_rng(seed)
    seq = [int(rng.integers(0, 5000)) for _ in range(A_ROWS)]       # every sender's next packet number
    seq[1], seq[2] = 3, 10
    first_seq = dict()                                              # the first packet number a sender sent while selected
    ticks = []
    for t in range(A_TICKS):
        room = list(A_ROOM_OF)
        if t >= A_MOVE_TICK:
            room[A_MOVER] = 4
        sel = [0] * A_ROWS
        sel[0] = 1                                                   # alone in its room: forwarded to nobody
        sel[1], sel[2] = (1, 0) if t < 5 else (0, 1)                 # room 1: the slot goes from row 1 to row 2, high up
        for x in (3, 4, 5):                                          # room 2: all three talk, K of them hold slots
            sel[x] = 1 if t not in (4,) else int(x != 3)
        sel[A_MOVER] = 1                                             # the mover talks throughout
        sel[7] = int(t % 3 != 2)
        sel[11] = int(t < 4 or t >= 7)                               # stops and returns
        for x in (12, 13, 14, 15):                                   # with row 11 (and the mover) more than K in room 4
            sel[x] = int(t >= 1)
        sel[16] = int(t >= 2)                                        # selected, but silent until tick 5: no slot before that
        sel[23] = 1                                                  # in no room
        arr, lev = [], []
        for x in range(A_ROWS):
            burst = int(rng.integers(0, 4))
            if x == 16 and t < 5:
                burst = 0
            if x in (1, 2, A_MOVER, 12) and burst == 0:
                burst = 1
            if x == 1 and t == 3:                                    # a jump to the top of the range: forwarded, next = 2^31 - 3
                seq[1] = TOP
            if x == 1 and t == 4:
                burst = 0
            if x == 2 and t == 5:
                seq[2], burst = 10, 3                                # 10, 11, 12 -> 2^31 - 3, 2^31 - 2 and one beyond the top
            for _ in range(burst):
                descs = [(0, 1), (0,), (1,)][int(rng.integers(0, 3))]
                for d in descs:
                    ln = int(rng.integers(1, 200))
                    arr.append((x, seq[x], d if rng.integers(0, 12) else -1, int(rng.integers(0, 60000)), ln))
                    lev.append(int(rng.integers(0, 256)) if rng.integers(0, 4) else 255)
                if sel[x] and x not in first_seq:
                    first_seq[x] = seq[x]
                seq[x] = min(seq[x] + 1, TOP)
            if sel[x] and x in first_seq and first_seq[x] > 0 and t % 4 == 3 and x not in (1, 2):   # late: below where its slot began
                arr.append((x, first_seq[x] - 1, 0, 7, 33))
                lev.append(255)
            if not sel[x]:
                first_seq.pop(x, None)
        for _ in range(int(rng.integers(1, 4))):                     # what solo_rtp_parse rejected, and a stream beyond n
            arr.append((-1, 0, 0, 0, 0))
            lev.append(255)
        arr.append((A_ROWS + 3, 5, 0, 0, 9))
        lev.append(17)
        order = rng.permutation(len(arr))
        ticks.append(dict(arrivals=np.array([arr[i] for i in order], np.int64).astype(np.int32).reshape(-1, 5), level_in=np.array([lev[i] for i in order], np.uint8),
                          default_level=(255, 0x7F, 200)[t % 3], sel=np.array(sel, np.uint8), room=np.array(room, np.int32),
                          cut=("all", "mid", "all", "zero")[t % 4]))
    return ticks


B_ROWS = 700


def scenario_b(seed):
    """three ticks of ONE room of 700 members (past 64 and 256 lanes), five to seven selected, K = 3"""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 100000, B_ROWS).tolist()
    talk = [[5, 64, 300, 511, 699], [5, 63, 64, 256, 300, 699], [0, 64, 255, 256, 640, 699, 300]]
    ticks = []
    for t in range(3):
        sel = np.zeros(B_ROWS, np.uint8)
        sel[talk[t]] = 1
        arr, lev = [], []
        for x in sorted(set(talk[t]) | {1, 2, 698}):
            for _ in range(int(rng.integers(1, 3)) if not (t == 0 and x == 300) else 0):
                for d in (0, 1):
                    arr.append((x, seq[x], d, int(rng.integers(0, 60000)), int(rng.integers(1, 200))))
                    lev.append(int(rng.integers(0, 255)))
                seq[x] += 1
        order = rng.permutation(len(arr))
        ticks.append(dict(arrivals=np.array([arr[i] for i in order], np.int32).reshape(-1, 5), level_in=np.array([lev[i] for i in order], np.uint8),
                          default_level=255, sel=sel, room=np.zeros(B_ROWS, np.int32), cut=("all", "mid", "all")[t]))
    return ticks


def permuted(tick, rng):
    """the same tick with its arrivals in another order"""
    order = rng.permutation(tick["arrivals"].shape[0])
    return dict(tick, arrivals=np.ascontiguousarray(tick["arrivals"][order]), level_in=np.ascontiguousarray(tick["level_in"][order]))


def run(model, ticks, n, n_rooms, call, cut_all=False):
    """Every tick through the model and through call(tick, rowinfo_words, max_records) -> dict(rowinfo, sa, level, records, send_count,
    count, level_fwd, slot_src, state) of the implementation under test, compared field for field -> the model's results per tick.
    cut_all: every tick with room for all its records."""
    out = []
    for t, tick in enumerate(ticks):
        rows = levels(tick["arrivals"], tick["level_in"], n, tick["default_level"])
        res = model.route(tick["arrivals"], rows, tick["sel"], tick["room"], n, n_rooms)
        assert res is not None
        mr = len(res["records"]) + 5
        if not cut_all and tick["cut"] == "zero":
            mr = 0
        elif not cut_all and tick["cut"] == "mid":
            mr = mid_arrival_cut(res)
            assert mr is not None and 0 < mr < len(res["records"]), (t, mr)
        want_rec, want_send = cut(res, mr)
        got = call(tick, rowinfo_words(rows), mr)
        assert np.array_equal(got["rowinfo"], rowinfo_words(rows)), (t, "rowinfo")
        assert got["sa"].tolist() == [r["sa"] for r in rows] and got["level"].tolist() == [r["level"] for r in rows], (t, "sa / level")
        assert got["count"] == res["count"], (t, got["count"], res["count"])
        assert got["send_count"] == want_send, (t, got["send_count"], want_send)
        assert np.array_equal(got["records"][:mr][:want_send["records"]], want_rec), (t, "records")
        assert (got["records"][want_send["records"]:] == got["fill32"]).all(), (t, "records behind the written ones")
        lf = np.full(got["level_fwd"].shape, got["fill8"], np.int64)
        for i, b in res["level_fwd"].items():
            lf[i] = b
        assert np.array_equal(got["level_fwd"], lf), (t, "level_fwd")
        assert got["slot_src"].tolist() == res["slot_src"], (t, got["slot_src"].tolist(), res["slot_src"])
        assert np.array_equal(got["state"], model.state()), (t, "state")
        out.append(res)
    return out
