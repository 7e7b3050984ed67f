"""Planning of one batched ssr_conv2d_wgrad launch: pure arithmetic over the layer and item records (hip.WgradLayer, hip.WgradItem).

No torch, no device, no library call: the tile counts of the kernels and the CU / XCD counts of the device are arguments.
engine.WgradBatch owns the device side (tables, partial buffers, twin planes, launch) and calls these in finalize():
  cut      one layer -> (co, ci, pixel-range) items
  pair     two 32-channel output blocks over the same input patch -> one item
  balance  pixel-range granularity chosen by simulating the launch (cost, makespan)
  ORDERS   the launch order of the items, by name (SSR_WGRAD_ORDER)
"""
import heapq

from .hip import WgradItem

# cycles per 16 x 16-pixel tile and per write-out of the bf16 3x3 kernel (tools/wgrad_body_probe.hip, MI355X): the loaders'
# fetch rate (~12.5 B/clk per CU) bounds both kinds of item, so a single costs 3/4 of a pair for at most half of its products
COST_TILE = {2: 5900, 1: 4300}
COST_WRITEOUT = 25000


def cut(entries, cout, cin_w, ci_tile, tiles, atomic):
    """The items of one layer: every (32 output channels, `ci_tile` input channels) tile of its weight, each over len(entries) pixel
    ranges of its `tiles` pixel tiles.  entries[sp] is the layer-table entry range sp writes to (the layer itself, or its per-split
    entry of the deterministic mode)."""
    per = -(-tiles // len(entries))
    out = []
    for co0 in range(0, cout, 32):
        for ci0 in range(0, cin_w, ci_tile):
            for sp, li in enumerate(entries):
                b, e = sp * per, min(tiles, (sp + 1) * per)
                if b < e:
                    out.append(WgradItem(li, co0, ci0, b, e, atomic, 1, li, co0))
    return out


def weight(layers, it):
    """MFMA work of an item in (tile, 32-ci half, 32-co plane) units"""
    return (it.tile_end - it.tile_begin) * (2 if layers[it.layer].Cin_w - it.ci0 > 32 else 1) * max(1, it.nco)


def cost(it):
    nco = max(1, it.nco)
    return (it.tile_end - it.tile_begin) * COST_TILE[nco] + nco * COST_WRITEOUT


def makespan(items, n_cu):
    """workgroups are handed to the CUs in index order as CUs become free: list scheduling, longest first"""
    free = [0] * n_cu
    for c in sorted((cost(it) for it in items), reverse=True):
        heapq.heapreplace(free, free[0] + c)
    return max(free)


def balance(items, n_cu):
    """Pixel-range granularity of the items, chosen by simulating the launch: a generator launch is ~2.2 paired items per
    CU, and whole items left 19 % of the CU time idle at the end (the singles, 3/4 of a pair each, are dealt last).  Finer
    items cost a write-out each (fp32 atomics of the whole (co, ci) tile), so the cut is as coarse as the simulation allows.
    -> (items, (t_pair, t_single, makespan, makespan of the items as given))"""
    def recut(t_pair, t_single):
        out = []
        for it in items:
            n, t = it.tile_end - it.tile_begin, (t_pair if it.nco == 2 else t_single)
            parts = max(1, -(-n // t))
            per = -(-n // parts)
            for b in range(it.tile_begin, it.tile_end, per):
                out.append(WgradItem(it.layer, it.co0, it.ci0, b, min(it.tile_end, b + per), 1 if parts > 1 else it.atomic,
                                     it.nco, it.layer_b, it.co0_b))
        return out
    best = None
    for t_pair in (128, 64, 32):
        for t_single in (128, 64, 32, 16):
            cand = recut(t_pair, t_single)
            m = makespan(cand, n_cu)
            if best is None or m < best[0] * 0.98:         # finer only if it buys 2 %
                best = (m, cand, t_pair, t_single)
    return best[1], best[2:] + (best[0], makespan(items, n_cu))


def pair(layers, items):
    """Two 32-channel blocks of output gradients that are contracted with the SAME input patch share one work item
    (csrc/wgrad_bf16.hip, Wg3: every X fragment read from LDS then feeds two MFMAs).  Same x view, ci0, geometry, pixel
    tiles and the same number of valid input channels; the blocks may belong to different layers — a dense block's
    conv1..conv4 all read x and produce dpre1..dpre4 (rrdbnet_arch.py:37-41) — or be the halves of one 64-output conv."""
    groups = {}
    for it in items:
        L = layers[it.layer]
        key = (L.x.p, L.x.cs, L.x.coff, it.ci0, it.tile_begin, it.tile_end, L.N, L.Hi, L.Wi, L.up, L.Gh, L.Gw, L.pad_y, L.pad_x,
               min(64, L.Cin_w - it.ci0) > 32, min(64, L.Cin - it.ci0), it.atomic)
        groups.setdefault(key, []).append(it)
    out = []
    for g in groups.values():
        for a, b in zip(g[0::2], g[1::2]):
            out.append(WgradItem(a.layer, a.co0, a.ci0, a.tile_begin, a.tile_end, a.atomic, 2, b.layer, b.co0))
        if len(g) % 2:
            out.append(g[-1])
    return out


def buffer_groups(layers, items):
    """the items that read one input buffer over the same pixel tiles, in order of first appearance"""
    groups = {}
    for it in items:
        groups.setdefault((layers[it.layer].x.p, it.tile_begin, it.tile_end), []).append(it)
    return list(groups.values())


def order_heavy(layers, items, n_xcd):
    """longest first only (rounds 3-5)"""
    return sorted(items, key=lambda it: -cost(it))


def order_xcd(layers, items, n_xcd):
    """Workgroup b runs on XCD b % 8 and every XCD has its own L2.  Items that read the same input buffer over the same
    pixel tiles (a dense block: 14 (conv, co, ci) items over one 192-channel buffer and its gradient) are dealt to ONE
    XCD, next to each other in its queue, so that they walk the tiles together and a line of x / dy is fetched once per
    group instead of once per item (layer-major order spread the 14 over all eight L2s: 3.39 GB per launch for
    ~0.6 GB of distinct lines, profiles/r03k_traffic.json)."""
    w = lambda it: weight(layers, it)      # noqa: E731
    queues, load = [[] for _ in range(n_xcd)], [0] * n_xcd
    for g in sorted(buffer_groups(layers, items), key=lambda g: -sum(map(w, g))):      # heaviest group first, to the least loaded XCD
        q = min(range(n_xcd), key=lambda j: (load[j], j))
        queues[q] += sorted(g, key=lambda i: -w(i))
        load[q] += sum(map(w, g))
    # block index = 8 * position + xcd has to be dense: level the queue lengths with items from the tails
    while True:
        lo, hi = min(queues, key=len), max(queues, key=len)
        if len(hi) - len(lo) <= 1:
            break
        lo.append(hi.pop())
    queues.sort(key=lambda q: -len(q))
    return [q[j] for j in range(len(queues[0])) for q in queues if j < len(q)]


def order_hybrid(layers, items, n_xcd):
    """Longest items first - what list scheduling over 256 CUs needs - and INSIDE every run of equal-cost items (a generator launch is a few
    cost classes of hundreds of identical items: the dense blocks are all alike) the items that read the same buffers over the same tiles are
    dealt to ONE XCD (block b runs on XCD b % 8), next to each other in its queue: the L2 saving of `order_xcd` (round 6: 4.43 -> 3.02 GB of
    HBM reads per 3x3 launch) without its cost (+0.7 ms per step: whole groups per XCD unbalance the tail)."""
    items = order_heavy(layers, items, n_xcd)
    out = []
    i = 0
    while i < len(items):
        c = cost(items[i])
        j = i
        while j < len(items) and cost(items[j]) == c:
            j += 1
        queues = [[] for _ in range(n_xcd)]
        for g in sorted(buffer_groups(layers, items[i:j]), key=len, reverse=True):
            min(queues, key=len).extend(g)
        for pos in range(len(out), len(out) + (j - i)):
            q = queues[pos % n_xcd]
            if not q:
                q = max(queues, key=len)
            out.append(q.pop(0))
        i = j
    return out


# hybrid (default since round 6): longest items first, equal-cost runs dealt to the XCDs by buffer group - 4.44 -> 3.09 GB of HBM reads per
# 3x3 launch at the same step time (25.36 / 25.42 / 25.40 against 25.40 / 25.46 / 25.35 ms, call r06x3); heavy: longest first only;
# xcd: whole buffer groups per XCD (3.02 GB, +0.7 ms per step: the tail is unbalanced)
ORDERS = {"hybrid": order_hybrid, "xcd": order_xcd, "heavy": order_heavy}
