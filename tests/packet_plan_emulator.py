"""Python emulation of k_packet_plan (gtcrn_packet_stream_*_slots, include/gtcrn_micro_hip.h "packet stream slots"): the
per-slot phases, the hops each named row steps, and the per-round tables in the call's row order.  Test infrastructure:
the CPU suite checks it against gtcrn_packet_stream_schedule, the GPU suite uses it to state what a schedule contains."""
from math import gcd


def hmax_of(n16):
    return (256 - gcd(n16, 256) + n16) // 256


def plan(phase, slots, count, n16, max_active=None):
    """One call.  phase: list of per-slot phases (advanced IN PLACE for the rows that step); slots: the call's table;
    count: the device count (clamped to 0..max_active).  Returns (h, tabs, pos, old): per stepping row its hops and old
    phase, per round r < hmax the table of slots with h > r in row order, and per round the rows' places (-1: none)."""
    m = len(slots) if max_active is None else max_active
    n = min(max(count, 0), m)
    hm = hmax_of(n16)
    h, old = [], []
    for i in range(n):
        phi = phase[slots[i]]
        assert 0 <= phi < 256 and phi % gcd(n16, 256) == 0
        old.append(phi)
        h.append((phi + n16) // 256)
        phase[slots[i]] = (phi + n16) % 256
    tabs, pos = [], []
    for r in range(hm):
        tab, p = [], []
        for i in range(n):
            if h[i] > r:
                p.append(len(tab))
                tab.append(slots[i])
            else:
                p.append(-1)
        tabs.append(tab)
        pos.append(p)
    assert all(x <= hm for x in h)
    return h, tabs, pos, old


def run(nslots, schedule, n16):
    """schedule: per tick the list of slots named (all count).  Slots start at phase 0.  Returns per tick the plan's h."""
    phase = [0] * nslots
    return [plan(phase, ids, len(ids), n16)[0] for ids in schedule], phase
