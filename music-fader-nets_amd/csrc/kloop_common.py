"""What gen_kloop.py, gen_kloop2.py, gen_kloop3.py and gen_kloop4.py share: the in-order model behind every hand-counted `s_waitcnt vmcnt(n)` and the
text of one asm statement.  (check_kloops.py does NOT import this on purpose: it re-derives the counts from the header text.)"""

SB = 84              # s84:85 = running operand base, s86:87 = saved exec / scratch (all clobbered)
UB = 3072            # bf16 x 6: bytes of one unit on the exchange slab / in the weight image (3 pieces x 1 KB)
PROD = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]      # bf16 x 6: (piece of A, piece of B = weights), smallest product first; 0 = hi, 1 = mid, 2 = lo
SLAB = ("store", "slab")                                     # queue key of an exchange-slab store (what an arrival waits for)


def rng(r, n=4, f="a"):
    """register range: a[r:r+n-1]"""
    return "%s[%d:%d]" % (f, r, r + n - 1)


def clobber(f, regs):
    return ['"%s%d"' % (f, i) for i in regs]


def advance(nbytes=0x1000, nop=False):
    """scalar operand base += nbytes; nop: a vector-memory instruction follows at once (SALU write of the base -> VMEM read of it)"""
    return ["s_add_u32 s%d, s%d, 0x%x" % (SB, SB, nbytes), "s_addc_u32 s%d, s%d, 0" % (SB + 1, SB + 1)] + (["s_nop 4"] if nop else [])


def lanes32(ins, on=True):
    """ins executed by lanes 0-31 only (64-row groups: every wave's epilogue items sit there)"""
    if not on:
        return ins
    return ["s_mov_b64 s[%d:%d], exec" % (SB + 2, SB + 3), "s_mov_b64 exec, 0xffffffff"] + ins + ["s_mov_b64 exec, s[%d:%d]" % (SB + 2, SB + 3)]


class Slots:
    """one pipeline unit: what is issued behind each of its MFMAs, every instruction together with the key it enters the queue under"""

    def __init__(self, nmf):
        self.at = [[] for _ in range(nmf)]

    def put(self, t, ins, key=None):
        """ins (one instruction, or a list that issues ONE memory operation) goes behind MFMA t; key = None: no vector-memory operation"""
        self.at[t].append(([ins] if isinstance(ins, str) else list(ins), key))


class VmQueue:
    """Vector-memory operations retire in order on vmcnt: an operation has completed once `s_waitcnt vmcnt(n)` returns with n = the number of operations
    issued BEHIND it.  self.ops = keys of everything issued so far, oldest first, starting with what is in flight when the statement begins."""

    def __init__(self, in_flight=()):
        self.ops = list(in_flight)
        self.n0 = len(self.ops)

    def issue(self, key):
        self.ops.append(key)

    def wait(self, n):
        assert n < 64, n         # the vmcnt field of gfx950 holds 0..63 (the generators had 60, 62 and 64 here: no statement comes near any of them)
        return "s_waitcnt vmcnt(%d)" % n

    def wait_for(self, key):
        """the YOUNGEST operation issued under key has completed"""
        last = max(i for i, o in enumerate(self.ops) if o == key)
        return self.wait(len(self.ops) - 1 - last)

    def wait_slab_store(self):
        """arrival: the statement's last exchange-slab store has completed; without one, everything older than the statement has"""
        return self.wait_for(SLAB) if SLAB in self.ops[self.n0:] else self.wait(len(self.ops) - self.n0)

    def unit(self, mfmas, slots, tail=(), t_tail=0):
        """text of one unit.  The queue lists its operations in the order of their MFMA slots - the ISSUE order - whatever order they were put in (round 5:
        listed in append order, the arrival waits of fn_rs_bwd_t1_main / fn_pp_bwd_k768_main were one too lenient).  tail: scalar bookkeeping for the next
        unit, one instruction (or s_add / s_addc pair) per MFMA gap from t_tail on that is otherwise free (the last gap takes one anyway), the rest behind"""
        out, tail = [], list(tail)
        for t, mf in enumerate(mfmas):
            out.append(mf)
            for ins, key in slots.at[t]:
                out += ins
                if key is not None:
                    self.ops.append(key)
            if tail and t >= t_tail and (not slots.at[t] or t == len(mfmas) - 1):
                out.append(tail.pop(0))
                if tail and tail[0].startswith("s_addc"):
                    out.append(tail.pop(0))
        return out + tail


def statement(comment, name, sig, pre, lines, outs, ins, clobbers):
    """C++ text of one function around one asm statement; pre = C++ lines in front of it, outs / ins = constraint lists, clobbers = list of quoted names"""
    body = "\n".join('        "%s\\n\\t"' % l for l in lines)
    return "\n%s\nFN_DEVINL void %s(%s) {\n%s    asm volatile(\n%s\n%s\n        : %s\n        : %s);\n}\n" % (
        comment, name, sig, "".join("    %s\n" % p for p in pre), body, ("        : " + outs).rstrip(), ins, ", ".join(clobbers))
