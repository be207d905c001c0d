"""A happens-before checker over the logs of tests/progs/coll_trace.c.

The logs of the N ranks of one run (test_rccl_sequence_cpu.run_plan) name every
device operation csrc/host/coll_hip.c issues with its buffers, stream and
events.  analyse() builds the happens-before order of those operations and
returns every violation of the rules below; check_order() raises on the first
run that has one.

Model.  One node per device operation, in host issue order per rank, with a
stream and the byte ranges it reads and writes (element size from the plan
line's type):
  memcpy        reads src, writes dst
  reduce_local  reads in, reads and writes io
  combine       reads every in=, writes out
  group         one RCCL group (group_start .. group_end) is one node with a
                start and an end: its sends read, its recvs write
  allreduce / reduce_scatter / reduce (the stub's collectives): one node each
Order.  Nodes on one stream of a rank: by issue.  event_record e s remembers
s's position, stream_wait s e puts later nodes on s after the latest record of
e (no record: an error).  stream_sync s / device_sync put everything issued
before on s / on every stream of the rank before everything issued after, on
any stream.  Across ranks: everything before a's group start happens before
the end of the group of every rank b that receives from a in that group (not
the other way: a send may complete from a buffer); a stub collective has that
edge from every rank's start to every rank's end.  Groups and collectives are
matched by their position in the logs, as test_rccl_sequence_cpu.check() does.
Buffers: scratch<k> for the life of the process; send / recv per call
(`note call <n>`): the harness reserves them anew.

Rules (Violation.rule):
  1 no race: two nodes of a rank touch overlapping bytes, one writes: the
    earlier-issued happens before the later.
  2 entry: on a caller's stream the call's accesses to send / recv are after a
    virtual producer at the head of the call on that stream.
  3 exit: on a caller's stream they are before a virtual consumer on that
    stream behind the call; on the communicator's stream they are
    host-complete before the next call.
  4 scratch carries nothing across calls: every scratch byte read was written
    by a node of the same call (that it is ordered after the read is rule 1).
  5 no free under use: at `free scratch<k>` every node that touched it is
    host-complete.
  6 the stated contract (include/mpix_hip_coll.h, Streams): between two
    consecutive calls of a communicator on different streams the caller has
    completed the earlier one.  The checker inserts that synchronisation.

Implementation: vector clocks with one component per (rank, stream).  A node
is (component, tick); `clock[c] >= tick` says it happens before whatever holds
that clock.  `host` is what the host has waited for.
"""
import collections

ESZ = {"f16": 2, "f32": 4, "f64": 8, "i32": 4}
INF = 1 << 62
RULES = {1: "no race", 2: "entry", 3: "exit", 4: "scratch carried across calls", 5: "free under use",
         0: "malformed log"}

Violation = collections.namedtuple("Violation", "rule rank call first second buf lo hi")


def describe(v):
    rng = f"{v.buf}[{v.lo},{'end' if v.hi >= INF else v.hi})" if v.buf else ""
    return (f"rule {v.rule} ({RULES[v.rule]}): rank {v.rank} call {v.call}: `{v.first}` not ordered before "
            f"`{v.second}` {rng}")


class OrderError(AssertionError):
    pass


def join(into, other):
    for k, t in other.items():
        if into.get(k, 0) < t:
            into[k] = t


class Access:
    __slots__ = ("lo", "hi", "write", "comp", "tick", "call", "line", "virtual")

    def __init__(self, lo, hi, write, node):
        self.lo, self.hi, self.write = lo, hi, write
        self.comp, self.tick, self.call, self.line, self.virtual = node


def ptr(text):
    """<base>+<offset> of the log -> (base, offset); None for null."""
    if text == "null":
        return None
    base, _, off = text.partition("+")
    return base, int(off)


def fields(tokens):
    return dict(t.split("=", 1) for t in tokens if "=" in t)


class Rank:
    def __init__(self, rank, log, out):
        self.rank, self.log, self.out = rank, log, out
        self.pos = 0
        self.clock = {}                 # stream -> vector clock
        self.host = {}
        self.events = {}
        self.ticks = collections.Counter()
        self.hist = collections.defaultdict(list)       # buffer key -> [Access]
        self.call, self.call_stream, self.esz = -1, None, 4
        self.group = None               # accesses of the open group

    # ---- clocks
    def comp(self, stream):
        return (self.rank, stream)

    def at(self, stream):
        """The clock of the next operation on `stream`."""
        c = self.clock.setdefault(stream, {})
        join(c, self.host)
        return c

    def node(self, stream, line, virtual=None):
        c = self.at(stream)
        k = self.comp(stream)
        self.ticks[k] += 1
        return c, (k, self.ticks[k], self.call, line, virtual)

    def done(self, clock, node):
        clock[node[0]] = node[1]

    def complete(self, a):
        return self.host.get(a.comp, 0) >= a.tick

    # ---- buffers
    def key(self, base):
        return (base, self.call) if base in ("send", "recv") else base

    def report(self, rule, first, second, buf, lo, hi):
        self.out.append(Violation(rule, self.rank, self.call, first, second, buf if isinstance(buf, str) else buf[0],
                                  lo, hi))

    def touch(self, clock, node, base, lo, hi, write):
        """One access of `node` (pre-clock `clock`) checked against the history
        of its buffer and entered into it."""
        if hi <= lo:
            return
        key = self.key(base)
        hist, keep = self.hist[key], []
        if not write and base.startswith("scratch"):
            self.rule4(hist, node, base, lo, hi)
        for a in hist:
            if a.hi <= lo or a.lo >= hi or (a.comp == node[0] and a.tick == node[1]):
                keep.append(a)
                continue
            ordered = clock.get(a.comp, 0) >= a.tick
            if (write or a.write) and not ordered:
                rule = 2 if a.virtual == "producer" else 3 if node[4] == "consumer" else 1
                self.report(rule, a.line, node[3], key, max(lo, a.lo), min(hi, a.hi))
            # an access that the new one covers and follows is represented by
            # it from here on (a later conflict with the old one is a conflict
            # with the new one); what sticks out of the new range stays
            if write or (not a.write and ordered):
                if a.lo < lo:
                    b = Access(a.lo, lo, a.write, (a.comp, a.tick, a.call, a.line, a.virtual))
                    keep.append(b)
                if a.hi > hi:
                    b = Access(hi, a.hi, a.write, (a.comp, a.tick, a.call, a.line, a.virtual))
                    keep.append(b)
            else:
                keep.append(a)
        keep.append(Access(lo, hi, write, node))
        self.hist[key] = keep

    def rule4(self, hist, node, base, lo, hi):
        # the write entries of a history never overlap: each byte's latest writer
        cover = sorted((max(a.lo, lo), min(a.hi, hi), a) for a in hist if a.write and a.lo < hi and a.hi > lo)
        at = lo
        for wlo, whi, a in cover:
            if wlo > at:
                self.report(4, "(no write)", node[3], base, at, wlo)
            if a.call != self.call:
                self.report(4, f"call {a.call}: {a.line}", node[3], base, wlo, whi)
            at = max(at, whi)
        if at < hi:
            self.report(4, "(no write)", node[3], base, at, hi)

    def op(self, stream, line, reads, writes):
        clock, node = self.node(stream, line)
        for base, lo, hi in reads:
            self.touch(clock, node, base, lo, hi, False)
        for base, lo, hi in writes:
            self.touch(clock, node, base, lo, hi, True)
        self.done(clock, node)

    # ---- calls
    def end_call(self):
        if self.call < 0:
            return
        keys = [("send", self.call), ("recv", self.call)]
        if self.call_stream == "user":
            clock, node = self.node("user", f"(consumer behind call {self.call})", "consumer")
            for key in keys:
                if self.hist.get(key):
                    self.touch(clock, node, key[0], 0, INF, True)
            self.done(clock, node)
        else:
            for key in keys:
                for a in self.hist.get(key, ()):
                    if not self.complete(a):
                        self.report(3, a.line, f"(host return of call {self.call})", key, a.lo, a.hi)
        for key in keys:
            self.hist.pop(key, None)

    def begin_call(self, n, detail):
        self.end_call()
        stream = fields(detail)["stream"]
        if self.call_stream is not None and stream != self.call_stream:
            for c in list(self.clock.values()):         # rule 6: the caller's synchronisation
                join(self.host, c)
        self.call, self.call_stream, self.esz = n, stream, ESZ[detail[1]]
        if stream == "user":
            clock, node = self.node("user", f"(producer ahead of call {n})", "producer")
            for base in ("send", "recv"):
                self.touch(clock, node, base, 0, INF, True)
            self.done(clock, node)

    # ---- the log
    def advance(self):
        """Runs the log up to the next group or stub collective: returns
        (kind, pre-clock copy, senders, clock, node) for the cross-rank join,
        or None at the end of the log."""
        log = self.log
        while self.pos < len(log):
            ev = log[self.pos]
            nxt = log[self.pos + 1] if self.pos + 1 < len(log) else []
            self.pos += 1
            kind = ev[0]
            if kind == "note":
                self.note(ev[1:], nxt)
            elif kind == "group_start":
                self.group = []
            elif kind in ("send", "recv"):
                f = fields(nxt)
                base, off = ptr(f["buf"])
                self.group.append((kind, int(ev[1]), int(ev[3]), base, off, f["stream"], " ".join(ev) + " " + f["buf"]))
            elif kind == "group_end":
                return self.close_group()
            elif kind in ("allreduce", "reduce_scatter", "reduce"):
                return self.collective(ev, fields(nxt))
            elif kind == "destroy":
                self.end_call()
                self.call = -1
        self.end_call()
        self.call = -1
        return None

    def close_group(self):
        xs, self.group = self.group, None
        streams = {x[5] for x in xs}
        if len(streams) > 1:
            self.report(0, "group", "transfers of one group on streams " + ",".join(sorted(streams)), "", 0, 0)
        stream = xs[0][5] if xs else self.call_stream_name()
        clock = self.at(stream)
        pre = dict(clock)
        k = self.comp(stream)
        self.ticks[k] += 1
        senders = set()
        for kind, nbytes, peer, base, off, _, line in xs:
            node = (k, self.ticks[k], self.call, line, None)
            self.touch(clock, node, base, off, off + nbytes, kind == "recv")
            if kind == "recv":
                senders.add(peer)
        return "group", pre, senders, clock, (k, self.ticks[k])

    def call_stream_name(self):
        # an empty group carries no stream: it sits on the call's stream (the
        # communicator's is the first one created)
        return "user" if self.call_stream == "user" else "s0"

    def collective(self, ev, f):
        kind, count = ev[0], int(ev[1])
        nbytes = count * self.esz
        n = int(self.log[0][2])
        stream = f["stream"]
        clock = self.at(stream)
        pre = dict(clock)
        k = self.comp(stream)
        self.ticks[k] += 1
        node = (k, self.ticks[k], self.call, " ".join(ev), None)
        sb, rb = ptr(f["sendbuf"]), ptr(f["recvbuf"])
        if sb:
            self.touch(clock, node, sb[0], sb[1], sb[1] + nbytes * (n if kind == "reduce_scatter" else 1), False)
        if rb:
            self.touch(clock, node, rb[0], rb[1], rb[1] + nbytes, True)
        return kind, pre, None, clock, (k, self.ticks[k])

    def note(self, ev, nxt):
        kind = ev[0]
        if kind == "call":
            self.begin_call(int(ev[1]), nxt[3:])
        elif kind == "memcpy":
            f = fields(nxt)
            nbytes = int(ev[1])
            (db, do), (sb, so) = ptr(f["dst"]), ptr(f["src"])
            self.op(f["stream"], " ".join(nxt[2:]), [(sb, so, so + nbytes)], [(db, do, do + nbytes)])
        elif kind == "reduce_local":
            f = fields(nxt)
            nbytes = int(ev[1]) * self.esz
            (ib, io_), (ob, oo) = ptr(f["in"]), ptr(f["io"])
            self.op(f["stream"], " ".join(nxt[2:]), [(ib, io_, io_ + nbytes), (ob, oo, oo + nbytes)],
                    [(ob, oo, oo + nbytes)])
        elif kind == "combine":
            f = fields(nxt)
            nbytes = int(ev[2]) * self.esz
            ob, oo = ptr(f["out"])
            reads = [(b, o, o + nbytes) for b, o in map(ptr, f["in"].split(","))]
            self.op(f["stream"], " ".join(nxt[2:]), reads, [(ob, oo, oo + nbytes)])
        elif kind == "event_record":
            self.events[ev[1]] = dict(self.at(ev[2]))
        elif kind == "stream_wait":
            if ev[2] not in self.events:
                self.report(0, "(no record)", " ".join(ev), "", 0, 0)
            else:
                join(self.clock.setdefault(ev[1], {}), self.events[ev[2]])
        elif kind == "stream_sync":
            join(self.host, self.clock.get(ev[1], {}))
        elif kind == "device_sync":
            for c in list(self.clock.values()):
                join(self.host, c)
        elif kind == "free":
            base = ptr(ev[1])[0]
            for a in self.hist.get(base, ()):
                if not self.complete(a):
                    self.report(5, a.line, " ".join(ev), base, a.lo, a.hi)
            self.hist.pop(base, None)


def analyse(logs):
    """Every violation in the N ranks' logs of one run."""
    out = []
    ranks = [Rank(r, log, out) for r, log in enumerate(logs)]
    while True:
        pend = [rk.advance() for rk in ranks]
        if all(p is None for p in pend):
            return out
        if any(p is None for p in pend) or len({p[0] for p in pend}) > 1:
            raise OrderError("the ranks' groups and collectives do not line up: " + str([p and p[0] for p in pend]))
        for b, (kind, _, senders, clock, node) in enumerate(pend):
            for a in (range(len(ranks)) if senders is None else sorted(senders)):
                if a != b:
                    join(clock, pend[a][1])
            clock[node[0]] = node[1]


def rules_of(violations):
    return sorted({v.rule for v in violations})


def check_order(logs, what=""):
    bad = analyse(logs)
    if bad:
        raise OrderError(f"{what}: {len(bad)} ordering violations, rules {rules_of(bad)}; the first:\n" +
                         "\n".join(describe(v) for v in bad[:8]))
