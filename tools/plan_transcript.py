"""Canonical text of what the launch plans emit: the contract for changes to engine.py, wgrad_plan.py and archs/l2_archs.py.

A plan is data - lists of C-ABI calls over descriptor records and tables - and building one launches nothing, so the text is the same
on a machine without a GPU (ParamStore(device="cpu")) and on the device.  For every configuration of CONFIGS x the arithmetic modes
that apply:
  1. every call of every launcher in order (fwd, bwd, each bwd_segments entry, every cached discriminator / object-branch plan):
     function, label, fork / join structure, scalar arguments, and every ABI field of a descriptor argument (floats by their bits);
  2. every weight-gradient batch: dtype, kdt, k, stride, layers, items in launch order, partial layout and reduce items, and the split
     tables / split list of the older fp32x3 form;
  3. every ParamStore: pack items in both directions, gather segments, spectral-norm items, pad, s2d, offsets.
An address is written as b<n>+<byte offset>: n numbers the allocations (torch storages reachable from the plans and stores) in order of
first appearance in the text, so neither the allocator nor the order in which a plan allocates shows.  The CU / XCD counts are pinned
to (256, 8).

  python tools/plan_transcript.py --golden tests/golden/launch_plans.json     # every switch setting in a fresh process
  python tools/plan_transcript.py --one                                       # this process's environment: {name: text} as JSON
  python tools/plan_transcript.py --show gen_train/fp32x3                     # one text on stdout

tests/test_launch_plans_host.py regenerates every text and compares it with the committed file (call count + sha256 per
configuration, the full text of FULL_TEXT); tests/test_gpu_launch_plans.py builds three of them on the device.

The ViT towers have a table of their own, TOWER_CONFIGS: the CLIPScore metric plan (family x tower_arithmetic x tower_attention, fed
bgr + normalize, and once the reference's raw feed) and the CLIP loss plan (siglip x tower_arithmetic x tower_attention; fwd_target,
fwd_fake, bwd and their concatenation as separate launchers) on two two-block towers (head dims 64 and 72) at B, H, W = 2, 10, 13.
Per configuration the text also lists the model's weights (key, shape, dtype; under exact arithmetic a sha256 over their bytes), the
element count of the plan's buffers and the loss plan's saved_bytes.  On the CPU the split weights are zeroed buffers of the packed
size (packing is a kernel); their addresses are canonical either way.

  python tools/plan_transcript.py --tower-golden tests/golden/tower_plans.json
  python tools/plan_transcript.py --show loss/split/mfma/d72

tests/test_tower_plans_host.py and tests/test_gpu_tower_plans.py hold vit_tower.py, clipscore_metric.py and clip_loss.py to that file.

The CNN feature backbones have the third table, BACKBONE_CONFIGS: the LPIPS metric plan (VGG16 under both feeds; AlexNet at its three
test sizes, under both feeds, and once with its 3 x 3 layers refused by ssr_conv2d) at N = 2 and the perceptual loss plan (fwd_target,
fwd, bwd; the shipped taps in every arithmetic mode, and in fp32 a truncated tap set, the style term with and without the feature term,
both normalisation switches and the deterministic loss flag) at B = 2, 16 x 32.  Per configuration the text lists every launcher, the
plan's ParamStore with a sha256 over its fp32 arena, every other device weight (key, shape, dtype, one sha256 over the bytes) and the
element count of every buffer the plan owns by attribute name; the file also holds the sha256 of three random states.  On the CPU
ParamStore.pack() (a kernel) is a no-op.

  python tools/plan_transcript.py --backbone-golden tests/golden/backbone_plans.json
  python tools/plan_transcript.py --show lpips/alex/64x64

tests/test_backbone_plans_host.py and tests/test_gpu_backbone_plans.py hold cnn_backbone.py, lpips_metric.py and perceptual.py to that file.
"""
import argparse
import bisect
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ["fp32", "bf16", "fp32x3", "fp32f", "fp32h"]
# several switches are read at import: each setting is a process of its own.  "" = nothing set
RUNS = ["", "SSR_WGRAD_CHUNKS=2", "SSR_WGRAD_PAIR=0", "SSR_WGRAD_BALANCE=1", "SSR_WGRAD_ORDER=xcd", "SSR_WGRAD_ORDER=heavy", "SSR_WGRAD_T3=32",
        "SSR_X3_WGRAD_FUSED=0,SSR_X3_WGRAD_FUSED4=0", "SSR_X3_CHAIN=1", "SSR_X3_FIXUP=1", "SSR_FUSED_RDB=0", "SSR_FUSED_RDB_BWD=0",
        "SSR_RDB_PREFETCH=1", "SSR_DETERMINISTIC=1"]
FULL_TEXT = "gen_train/fp32x3"
G_KW = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=2, num_grow_ch=32)
L2_KW = dict(in_channels=3, mask_channels=0, hidden_channels=32, out_channels=3, kernel_size=3, residual_layers=1, zoom_factor=4,
             sr_kernel_size=1, use_reference_frame=False, output_size=32)           # the tiny fixtures of tests/test_l2_host.py


# ---------------------------------------------------------------------------------------------------- canonical addresses
def _reachable(roots):
    """every torch.Tensor and engine.WgradBatch / ParamStore reachable from `roots` through containers, attributes and byref()"""
    import torch
    seen, tensors, stack = set(), [], list(roots)
    skip = (str, bytes, int, float, bool, type(None), type, types.ModuleType, types.FunctionType, types.BuiltinFunctionType, C._CFuncPtr)
    while stack:
        o = stack.pop()
        if id(o) in seen or isinstance(o, skip):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            tensors.append(o)
            stack.extend(getattr(o, "_ssr_bf16_planes", None) or ())
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set, frozenset)):
            stack.extend(o)
        else:
            stack.extend(getattr(o, "__dict__", {}).values())
            if hasattr(o, "_obj"):                     # ctypes.byref(x)
                stack.append(o._obj)
    return tensors


class Canon:
    """address -> 'b<n>+<offset>' by the allocation that contains it, n in order of first appearance"""

    def __init__(self, roots):
        spans = {}
        for t in _reachable(roots):
            s = t.untyped_storage()
            if s.nbytes():
                spans[s.data_ptr()] = max(spans.get(s.data_ptr(), 0), s.nbytes())
        self.starts = sorted(spans)
        self.sizes = [spans[a] for a in self.starts]
        self.ids = {}

    def __call__(self, p):
        if not p:
            return "null"
        p = int(p)
        i = bisect.bisect_right(self.starts, p) - 1
        if i < 0 or p >= self.starts[i] + self.sizes[i]:
            raise LookupError("address 0x%x lies in no allocation the plans hold" % p)
        n = self.ids.setdefault(self.starts[i], len(self.ids))
        return "b%d+%d" % (n, p - self.starts[i])


def _fbits(v):
    return "f:%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def _fmt_value(canon, ctype, v):
    from satlas_super_resolution_amd import hip
    if ctype is hip.View:
        return "(%s,%d,%d)" % (canon(v.p), v.cs, v.coff)
    if ctype is C.c_void_p:
        return canon(v)
    if ctype is C.c_float:
        return _fbits(v)
    if issubclass(ctype, C.Array):
        return "[" + ",".join(_fmt_value(canon, ctype._type_, x) for x in v) + "]"
    if issubclass(ctype, C.Structure):
        return fmt_struct(canon, v)
    return str(int(v))


def fmt_struct(canon, s):
    """every field of a ctypes record, in ABI order"""
    return "{" + " ".join("%s=%s" % (n, _fmt_value(canon, t, getattr(s, n))) for n, t in s._fields_) + "}"


def decode(tab, ctype, n):
    """the first n records of a descriptor table (host or device tensor)"""
    raw = tab.cpu().numpy().tobytes()
    return list((ctype * n).from_buffer_copy(raw[:n * C.sizeof(ctype)]))


# ---------------------------------------------------------------------------------------------------- the three parts
def fmt_launcher(canon, L, out, indent=""):
    """-> number of C-ABI calls"""
    from satlas_super_resolution_amd.engine import Launcher
    n = 0
    for fn, args, what in L.calls:
        if fn is Launcher.FORK:
            out.append("%sfork %r {" % (indent, what))
            n += fmt_launcher(canon, args[0], out, indent + "  ")
            out.append(indent + "}")
            continue
        if fn is Launcher.JOIN:
            out.append(indent + "join")
            continue
        n += 1
        types_ = fn.argtypes[:-1]                      # the last one is the stream
        assert len(types_) == len(args), (fn.__name__, len(types_), len(args))
        parts = []
        for i, (t, a) in enumerate(zip(types_, args)):
            if isinstance(t, type) and issubclass(t, C._Pointer):
                if a is None:
                    parts.append("null")
                elif isinstance(a, C.Array) and not issubclass(a._type_, C.Structure):      # scalars by value (perm, mean, std)
                    parts.append(_fmt_value(canon, type(a), a))
                elif isinstance(a, C.Array):           # (records, count)
                    parts.append("[" + " ".join(fmt_struct(canon, a[j]) for j in range(int(args[i + 1]))) + "]")
                else:
                    parts.append(fmt_struct(canon, a._obj))
            elif t is C.c_void_p:
                parts.append(canon(a))
            elif t is C.c_float:
                parts.append(_fbits(a))
            elif t is C.c_double:
                parts.append("d:%016x" % struct.unpack("<Q", struct.pack("<d", a))[0])
            elif isinstance(a, C.Structure):
                parts.append(_fmt_value(canon, t, a))
            else:
                parts.append(str(int(a)))
        out.append("%scall %s %r %s" % (indent, fn.__name__, what, " ".join(parts)))
    return n


def fmt_batch(canon, wb, out):
    from satlas_super_resolution_amd import hip
    out.append("batch dtype=%d kdt=%d k=%d stride=%d force_atomic=%d det=%d layers=%d items=%d"
               % (wb.dtype, wb.kdt, wb.k, wb.stride, int(wb.force_atomic), int(wb.det), len(wb.layers), len(wb.items)))
    for i, L in enumerate(wb.layers):
        out.append("  layer %d%s %s" % (i, " per-split" if i in wb.virtual else "", fmt_struct(canon, L)))
    for it in wb.items:
        out.append("  item " + fmt_struct(canon, it))
    for dw, db, wsize, bsize, lsp in wb._partials:
        out.append("  partial dw=%s db=%s wsize=%d bsize=%d entries=%s" % (canon(dw), canon(db), wsize, bsize, list(lsp)))
    if wb.partial is not None:
        out.append("  partials %s numel=%d n_reduce=%d max_reduce=%d" % (canon(wb.partial.data_ptr()), wb.partial.numel(), wb.n_reduce, wb.max_reduce))
        for r in decode(wb.reduce_tab, hip.ReduceItem, wb.n_reduce):
            out.append("  reduce " + fmt_struct(canon, r))
    for j, tab in enumerate(wb.split_tabs):
        for i, L in enumerate(decode(tab, hip.WgradLayer, len(wb.layers))):
            out.append("  split pass %d layer %d %s" % (j, i, fmt_struct(canon, L)))
    for p, h, l in wb.splits:
        out.append("  split %s -> %s %s numel=%d" % (canon(p.data_ptr()), canon(h.data_ptr()), canon(l.data_ptr()), p.numel()))
    if wb.split_tab is not None:
        for s in decode(wb.split_tab, hip.SplitItem, len(wb.splits)):
            out.append("  split item " + fmt_struct(canon, s))
    for name in ("layer_tab", "item_tab"):
        tab = getattr(wb, name)
        if tab is not None:
            out.append("  %s %s bytes=%d" % (name, canon(tab.data_ptr()), tab.numel()))


def fmt_store(canon, st, out):
    from satlas_super_resolution_amd import hip
    out.append("store %s dtype=%d fwd_dtype=%d numel=%d data=%s grad=%s"
               % (type(st).__name__, st.dtype, st.fwd_dtype, st.numel, canon(st.data.data_ptr()), canon(st.grad.data_ptr())))
    for k, (off, shape) in st.offsets.items():
        out.append("  offset %s %d %s" % (k, off, list(shape)))
    for k, v in st.pad.items():
        out.append("  pad %s %s s2d=%s" % (k, list(v), getattr(st, "s2d", {}).get(k)))
    for it in st._pack_items:
        out.append("  pack " + fmt_struct(canon, it))
    for it in getattr(st, "_pack_items_bwd", None) or ():
        out.append("  pack bwd " + fmt_struct(canon, it))
    for it in getattr(st, "_seg_items", ()):
        out.append("  gather seg " + fmt_struct(canon, it))
    for k, t in getattr(st, "gather", {}).items():
        out.append("  gather %s %s rows=%s" % (list(k), canon(t.data_ptr()), st.gather_rows.get(k)))
    for k, t in getattr(st, "repacked", {}).items():
        out.append("  repacked %s %s" % (list(k), canon(t.data_ptr())))
    if getattr(st, "sn_names", None):
        n = len(st.sn_names)
        out.append("  sn %s rows<=%d cols<=%d elems<=%d" % (",".join(st.sn_names), st.sn_max_rows, st.sn_max_cols, st.sn_max_elems))
        for it in decode(st.sn_table, hip.SNItem, n):
            out.append("  sn item " + fmt_struct(canon, it))
        for it in decode(st.sn_bwd_table, hip.SNBwdItem, n):
            out.append("  sn bwd item " + fmt_struct(canon, it))


def batches_of(plan):
    from satlas_super_resolution_amd.engine import WgradBatch
    out = []
    for p in getattr(plan, "parts", None) or [plan]:
        for attr in ("_wg_batches", "_keep", "wbatches"):
            out += [b for b in getattr(p, attr, None) or [] if isinstance(b, WgradBatch)]
    return out


def transcript(plans, stores, extra_roots=()):
    """plans: [(label, plan)] -> (text, number of C-ABI calls)"""
    canon = Canon([p for _, p in plans] + list(stores) + list(extra_roots))
    out, calls = [], 0
    for label, plan in plans:
        launchers = []
        for name in ("fwd", "bwd"):
            if getattr(plan, name, None) is not None:
                launchers.append((name, getattr(plan, name)))
        for i, (L, off, cnt) in enumerate(getattr(plan, "bwd_segments", None) or []):
            launchers.append(("bwd_segment %d offset=%d count=%d" % (i, off, cnt), L))
        for i, (key, L) in enumerate(getattr(plan, "_fwd_cache", {}).items()):
            launchers.append(("forward_plan %d x=%s" % (i, canon(key)), L))
        for i, (key, L) in enumerate(getattr(plan, "_bwd_cache", {}).items()):
            if len(key) == 4:
                key = "x=%s param_grads=%d input_grad=%d in_residual=%s" % (canon(key[0]), key[1], key[2], canon(key[3]))
            else:
                key = "param_grads=%d input_grad=%d" % (key[0], key[1])
            launchers.append(("backward_plan %d %s" % (i, key), L))
        for name, L in launchers:
            out.append("launcher %s %s" % (label, name))
            calls += fmt_launcher(canon, L, out, "  ")
    for label, plan in plans:
        for i, wb in enumerate(batches_of(plan)):
            out.append("wgrad %s %d" % (label, i))
            fmt_batch(canon, wb, out)
    for st in stores:
        fmt_store(canon, st, out)
    return "\n".join(out) + "\n", calls


# ---------------------------------------------------------------------------------------------------- configurations
def _gen(mode, dev, B=2, hw=16, det=False, split=False, **kw):
    import torch
    from satlas_super_resolution_amd import engine, hip
    net = dict(G_KW)
    net.update({k: kw.pop(k) for k in list(kw) if k in G_KW})
    st = engine.ParamStore(engine.generator_specs(**net), hip.dtype_code(mode), device=dev)
    extra = []
    with engine.deterministic_mode(det):
        if split:
            up = 1 << (3 if net["scale"] == 8 else 2)
            tdt = hip.torch_dtype(st.dtype)
            extra = [torch.zeros(B, hw * up, hw * up, 8, dtype=tdt, device=dev) for _ in range(2)]
            plan = engine.SplitGeneratorPlan(st, B, hw, hw, out_buf=extra[0], d_out_buf=extra[1], parts=2, training=True, **net, **kw)
            plans = [("split", plan)] + [("part%d" % i, p) for i, p in enumerate(plan.parts)]
        else:
            plans = [("g", engine.GeneratorPlan(st, B, hw, hw, **net, **kw))]
    return plans, [st], extra


def _disc(mode, dev, hw=128, cin=3, skip=True, det=False, B=2):
    import torch
    from satlas_super_resolution_amd import engine, hip
    code = hip.dtype_code(mode)
    st = engine.ParamStore(engine.discriminator_specs(cin, 64, in_hw=(hw, hw), dtype=hip.forward_code(code)), code, device=dev)
    with engine.deterministic_mode(det):
        plan = engine.DiscriminatorPlan(st, B, hw, hw, num_in_ch=cin, skip_connection=skip)
        tdt = hip.torch_dtype(st.dtype)
        x, res = (torch.zeros(B, hw, hw, engine.rup(cin, 8), dtype=tdt, device=dev) for _ in range(2))
        plan.forward_plan(x)
        plan.backward_plan(x, False, True, res)
        plan.backward_plan(x, True, False, None)
        plan.backward_plan(x, True, True, None)
    return [("d", plan)], [st], [x, res]


def _obj(mode, dev, hw=16):
    from satlas_super_resolution_amd import engine, hip
    st = engine.ParamStore(engine.object_branch_specs(), hip.F32, device=dev, extras=engine.object_branch_extras())
    plan = engine.ObjectBranchPlan(st, 3, hw, hw)
    plan.backward_plan(True, False)
    plan.backward_plan(False, True)
    return [("o", plan)], [st], []


def _l2(mode, dev, arch="SRCNN", revisits=4):
    import torch
    from collections import OrderedDict
    from satlas_super_resolution_amd.archs import l2_archs
    net = getattr(l2_archs, arch)(revisits=revisits, **L2_KW)
    if torch.device(dev).type == "cuda":
        st = net.to(dev).store()
    else:                                   # _L2Net.store() without its refusal of CPU parameters
        shapes = OrderedDict((k, tuple(p.shape)) for k, p in net.named_parameters())
        live = net.live_keys()
        convs = [k[:-len(".weight")] for k in live if k.endswith(".weight") and len(shapes[k]) == 4 and shapes[k][-1] == 3]
        st = net._store = l2_archs.L2Store(shapes, live, convs, dev)
    return [("l2", l2_archs.L2Plan(net, 2, 8, 8, True))], [st], []


class _Bare:
    """a launcher and its batch without a plan around them"""


def _wgrad_direct(mode, dev):
    """One weight-gradient batch over a buffer whose element count is no multiple of 8 (no plan has one: channels are padded to 8):
    the older fp32x3 form (SSR_X3_WGRAD_FUSED=0) then splits buffer by buffer, ssr_split_bf16 in place of ssr_split_bf16_multi."""
    import torch
    from satlas_super_resolution_amd import engine, hip
    x, dy, g = (torch.zeros(*s, device=dev) for s in ((1, 3, 3, 12), (1, 3, 3, 8), (8 * 12 * 9 + 8,)))
    p = _Bare()
    wb, p.bwd = engine.WgradBatch(hip.dtype_code(mode), 3, 1, device=dev), engine.Launcher()
    wb.add(hip.view(x), hip.view(dy), 1, 3, 3, 1, 12, 8, 3, 3, 1.0, g.data_ptr(), 12, g.data_ptr() + 4 * 8 * 12 * 9)
    wb.finalize()
    wb.launch(p.bwd)
    p._keep = [wb]
    return [("w", p)], [], [x, dy, g]


ALL, FP32 = tuple(MODES), ("fp32",)
CONFIGS = {      # name -> (builder, keyword arguments, modes)
    "gen_train": (_gen, dict(training=True, need_input_grad=True), ALL),
    "gen_atomic": (_gen, dict(training=True, need_input_grad=True, wgrad_atomic=True), ALL),
    "gen_split": (_gen, dict(B=4, split=True, need_input_grad=True), ALL),
    "gen_seg3": (_gen, dict(training=True, need_input_grad=True, bwd_segments=3, num_block=3), ALL),
    "gen_infer": (_gen, dict(training=False), ALL),
    "gen_scale2": (_gen, dict(training=True, need_input_grad=True, scale=2, hw=32), ALL),
    "gen_scale8": (_gen, dict(training=True, need_input_grad=True, scale=8), ALL),
    "gen_narrow": (_gen, dict(training=True, need_input_grad=True, num_feat=32, num_grow_ch=16), ALL),
    "gen_det": (_gen, dict(training=True, need_input_grad=True, det=True, B=4, hw=32, num_block=1), ALL),
    "disc_det": (_disc, dict(det=True), ALL),
    "obj16": (_obj, dict(hw=16), FP32),
    "obj32": (_obj, dict(hw=32), FP32),
    "l2_srcnn": (_l2, dict(arch="SRCNN", revisits=4), FP32),
    "l2_highresnet": (_l2, dict(arch="HighResNet", revisits=3), FP32),
    "wgrad_direct": (_wgrad_direct, {}, ("fp32x3",)),
}
for _hw in (64, 128):
    for _cin in (3, 6):
        for _skip in (True, False):
            CONFIGS["disc%d_in%d_%s" % (_hw, _cin, "skip" if _skip else "noskip")] = (_disc, dict(hw=_hw, cin=_cin, skip=_skip), ALL)
SWITCHED = ["gen_train", "disc128_in3_skip", "wgrad_direct"]         # what runs under every switch setting


def objects(name, mode, dev="cpu"):
    """([(label, plan)], stores, other buffers) of one configuration in this process's environment"""
    from satlas_super_resolution_amd import engine
    engine._device_cus = lambda: (256, 8)
    fn, kw, _ = CONFIGS[name]
    return fn(mode, dev, **kw)


def build(name, mode, dev="cpu"):
    """(text, calls) of one configuration in this process's environment"""
    return transcript(*objects(name, mode, dev))


def tables_of(plans, stores):
    """(what, device table, the host records it was made from) of every table the configuration owns"""
    out = []
    for label, plan in plans:
        for i, wb in enumerate(batches_of(plan)):
            if not wb.layers:
                continue
            out.append(("%s batch %d items" % (label, i), wb.item_tab, wb.items))
            if wb.split_tabs:
                out += [("%s batch %d split pass %d" % (label, i, j), t, h) for j, (t, h) in enumerate(zip(wb.split_tabs, wb.split_layers))]
            else:
                out.append(("%s batch %d layers" % (label, i), wb.layer_tab, wb.layers))
            if wb.reduce_tab is not None:
                out.append(("%s batch %d reduce" % (label, i), wb.reduce_tab, wb.reduce_items))
    for st in stores:
        out.append(("pack", st.pack_table, st._pack_items))
        if getattr(st, "_pack_items_bwd", None):
            out.append(("pack bwd", st.pack_table_bwd, st._pack_items_bwd))
    return out


def sweep(setting="", dev="cpu"):
    """{configuration/mode: (text, calls)} of this process: everything when nothing is set, else the SWITCHED ones"""
    out = {}
    for name in (SWITCHED if setting else CONFIGS):
        for mode in CONFIGS[name][2]:
            out["%s/%s" % (name, mode)] = build(name, mode, dev)
    return out


def sweep_in_subprocess(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SSR_")}
    env["OMP_NUM_THREADS"] = "1"            # the runs are side by side, and all they ask of torch is zeroed buffers
    for kv in filter(None, setting.split(",")):
        name, value = kv.split("=")
        env[name] = value
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--setting", setting], env=env, check=True,
                         capture_output=True, text=True).stdout
    return {(k if not setting else "%s [%s]" % (k, setting)): tuple(v) for k, v in json.loads(out).items()}


def all_runs(workers=8):
    """{configuration/mode [setting]: (text, calls)}, the settings side by side in fresh processes"""
    from concurrent.futures import ThreadPoolExecutor
    out = {}
    with ThreadPoolExecutor(max_workers=workers) as ex:
        for part in ex.map(sweep_in_subprocess, RUNS):
            out.update(part)
    return out


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


def golden(runs):
    doc = {"configs": {k: {"calls": c, "sha256": digest(t)} for k, (t, c) in runs.items()},
           "full_text": {FULL_TEXT: runs[FULL_TEXT][0].splitlines()}}
    return doc


# ---------------------------------------------------------------------------------------------------- the ViT towers
# The CLIPScore metric plan and the CLIP loss plan (vit_tower.py, clipscore_metric.py, clip_loss.py): a table of their own, recorded in
# tests/golden/tower_plans.json.  No switch is read at import, so one process builds them all.
TOWERS = {"d64": dict(width=128, depth=2, mlp=192, patch=4, grid=3, heads=2),           # head dim 64
          "d72": dict(width=144, depth=2, mlp=192, patch=4, grid=3, heads=2)}           # head dim 72, the other one both attention kernels take
TOWER_SHAPE = (2, 10, 13)            # B, H, W: not square, no multiple of the patch: both index tables and both inverse ranges are non-trivial
TOWER_FULL_TEXT = ("metric/siglip/split/mfma/d64", "loss/split/mfma/d72")
TOWER_CONFIGS = {}                   # name -> (builder, keyword arguments)


def _on_cpu(dev):
    import torch
    return torch.device(dev).type == "cpu"


class _cpu_pack:
    """on the CPU, linear_split.pack_split_weight (which launches ssr_linear_split_pack) gives a zeroed buffer of the packed size"""

    def __init__(self, dev):
        self.cpu = _on_cpu(dev)

    def __enter__(self):
        import torch
        from satlas_super_resolution_amd import hip, linear_split
        self.real = linear_split.pack_split_weight
        if self.cpu:
            linear_split.pack_split_weight = lambda w, pieces: torch.zeros(int(hip.lib().ssr_linear_split_pack_bytes(*w.shape)), dtype=torch.uint8)

    def __exit__(self, *exc):
        from satlas_super_resolution_amd import linear_split
        linear_split.pack_split_weight = self.real


def _metric_tower(dev, family, arithmetic, attention, tower, bgr=True, normalize=True):
    from satlas_super_resolution_amd import clipscore_metric as CM
    with _cpu_pack(dev):
        model = CM.CLIPVisualModel(CM.clip_random_state(family, **TOWERS[tower]), dev, tower_arithmetic=arithmetic, tower_attention=attention)
    plan = model.plan(*TOWER_SHAPE, bgr=bgr, normalize=normalize)
    return model, plan, [("launcher", plan.launcher)], []


def _loss_tower(dev, arithmetic, attention, tower):
    """fake, target and gradient views of channel stride 8, the target at channel offset 4 of the buffer it shares with the generated
    image; weight 0.5 into slot 0 of a slotted loss buffer"""
    import torch
    from satlas_super_resolution_amd import clip_loss as CL, clipscore_metric as CM, hip
    B, H, W = TOWER_SHAPE
    with _cpu_pack(dev):
        model = CL.ClipLossModel(CM.clip_random_state("siglip", **TOWERS[tower]), dev, tower_arithmetic=arithmetic, tower_attention=attention)
    images, grad = (torch.zeros(B, H, W, 8, device=dev) for _ in range(2))
    loss = torch.zeros(hip.LOSS_SLOTS, device=dev)
    plan = CL.ClipLossPlan(model, B, H, W, hip.View(images.data_ptr(), 8, 0), hip.View(images.data_ptr(), 8, 4), hip.View(grad.data_ptr(), 8, 0),
                           loss.data_ptr(), 0.5, hip.DETERMINISTIC)
    return model, plan, [(n, getattr(plan, n)) for n in ("fwd_target", "fwd_fake", "bwd", "launcher")], [images, grad, loss]


for _t in TOWERS:
    for _ar in ("exact", "split"):
        for _at in ("fma", "mfma"):
            for _f in ("siglip", "clip"):
                TOWER_CONFIGS["metric/%s/%s/%s/%s" % (_f, _ar, _at, _t)] = (_metric_tower, dict(family=_f, arithmetic=_ar, attention=_at, tower=_t))
            TOWER_CONFIGS["loss/%s/%s/%s" % (_ar, _at, _t)] = (_loss_tower, dict(arithmetic=_ar, attention=_at, tower=_t))
# the reference's feed: no mean / std (null pointers), the identity permutation
TOWER_CONFIGS["metric/siglip/exact/fma/d64/raw"] = (_metric_tower, dict(family="siglip", arithmetic="exact", attention="fma", tower="d64", bgr=False,
                                                                          normalize=False))


def tower_transcript(model, plan, launchers, extra):
    """-> (text, number of C-ABI calls): every launcher, then the (key, shape, dtype) of every weight the model holds - under exact
    arithmetic with a sha256 over the keys and bytes - the element count of the plan's buffers and the loss plan's saved_bytes"""
    canon = Canon([plan, model] + list(extra))
    out, calls = [], 0
    for name, L in launchers:
        out.append("launcher %s" % name)
        calls += fmt_launcher(canon, L, out, "  ")
    h = hashlib.sha256()
    for k in sorted(model.w):
        t = model.w[k]
        out.append("weight %s %s %s" % (k, list(t.shape), str(t.dtype).replace("torch.", "")))
        h.update(k.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    if model.tower_arithmetic == "exact":
        out.append("weights sha256 %s" % h.hexdigest())
    out.append("bufs numel %d" % sum(t.numel() for t in plan.bufs.values()))
    if hasattr(plan, "saved_bytes"):
        out.append("saved_bytes %d" % plan.saved_bytes)
    return "\n".join(out) + "\n", calls


def build_tower(name, dev="cpu"):
    """(text, calls) of one tower configuration"""
    fn, kw = TOWER_CONFIGS[name]
    return tower_transcript(*fn(dev, **kw))


def tower_sweep(dev="cpu"):
    return {name: build_tower(name, dev) for name in TOWER_CONFIGS}


def tower_golden(runs):
    return {"configs": {k: {"calls": c, "sha256": digest(t)} for k, (t, c) in runs.items()},
            "full_text": {k: runs[k][0].splitlines() for k in TOWER_FULL_TEXT}}


# ---------------------------------------------------------------------------------------------------- the CNN feature backbones
# The LPIPS metric plan (VGG16, AlexNet) and the perceptual loss plan (VGG19): cnn_backbone.py, lpips_metric.py, perceptual.py, recorded in
# tests/golden/backbone_plans.json.  The smallest shapes at which each branch is still taken.  AlexNet's three 3 x 3 layers go to
# ssr_conv2d at all three of the project's test sizes (grids of 1 x 1, 1 x 2 and 3 x 3), and at every other size: the pipelined family
# of csrc/conv.hip takes any grid of a 3 x 3 stride-1 layer in exact fp32 (pipe_shape_ok), so no image size makes ssr_conv2d_variant
# answer SSR_EUNSUP there (31 ... 299 a side were tried).  The plan's fallback to ssr_conv_direct is therefore recorded by the
# configuration lpips/alex/31x31/refused, in which the tool answers the plan's question with SSR_EUNSUP itself (_conv2d_refuses).
BACKBONE_N = 2
VGG_HW = (16, 32)                    # the smallest sides four poolings allow, and not square
SHIPPED_LAYER_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}        # options/*.yml
BACKBONE_FULL_TEXT = ("lpips/alex/64x64", "perceptual/fp32/style")
BACKBONE_CONFIGS = {}                # name -> (builder, keyword arguments)


class _no_pack:
    """on the CPU, ParamStore.pack() (which launches ssr_pack_weights) does nothing"""

    def __init__(self, dev):
        self.cpu = _on_cpu(dev)

    def __enter__(self):
        from satlas_super_resolution_amd import engine
        self.real = engine.ParamStore.pack
        if self.cpu:
            engine.ParamStore.pack = lambda store: None

    def __exit__(self, *exc):
        from satlas_super_resolution_amd import engine
        engine.ParamStore.pack = self.real


class _conv2d_refuses:
    """ssr_conv2d_variant answers SSR_EUNSUP (-2) for every descriptor, as if no kernel family took the grid"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from satlas_super_resolution_amd import hip
        self.real = hip.lib().ssr_conv2d_variant
        if self.on:
            hip.lib().ssr_conv2d_variant = lambda desc: -2

    def __exit__(self, *exc):
        from satlas_super_resolution_amd import hip
        hip.lib().ssr_conv2d_variant = self.real


def _lpips_backbone(dev, net, H, W, bgr=True, normalize=False, refused=False):
    from satlas_super_resolution_amd import lpips_metric as LM
    with _no_pack(dev):
        model = LM.LPIPSModel(LM.lpips_random_state(17, net), dev, net=net)
    with _conv2d_refuses(refused):
        plan = model.plan(BACKBONE_N, H, W, bgr=bgr, normalize=normalize)
    weights = [("lins", model.lins)]
    for name, (w, b) in (getattr(model, "direct", None) or {}).items():
        weights += [("direct.%s.weight" % name, w), ("direct.%s.bias" % name, b)]
    return plan, [("launcher", plan.launcher)], weights, []


def _perceptual_backbone(dev, mode, layer_weights=SHIPPED_LAYER_WEIGHTS, loss_flags=0, **opt):
    """generated image, target and gradient buffers of 8 channels; l_g_percep into the first half of a two-slot loss buffer, l_g_style into
    the second"""
    import torch
    from satlas_super_resolution_amd import hip, perceptual as P
    (H, W), code = VGG_HW, hip.dtype_code(mode)
    x, tgt, grad = (torch.zeros(BACKBONE_N, H, W, 8, dtype=hip.torch_dtype(hip.storage_code(code)), device=dev) for _ in range(3))
    loss = torch.zeros(2 * hip.LOSS_SLOTS, device=dev)
    opt = dict({"type": "PerceptualLoss", "layer_weights": dict(layer_weights), "vgg_type": "vgg19", "use_input_norm": True,
                "perceptual_weight": 1.0, "style_weight": 0, "range_norm": False, "criterion": "l1"}, **opt)
    state = P.vgg19_random_state(P.vgg19_specs(list(layer_weights)[-1]), 3)
    plan = P.PerceptualPlan(opt, BACKBONE_N, H, W, code, x, tgt, grad, loss.data_ptr(), state=state, loss_flags=loss_flags,
                            style_loss_ptr=loss.data_ptr() + 4 * hip.LOSS_SLOTS)
    if not _on_cpu(dev):
        plan.pack()
    return plan, [(n, getattr(plan, n)) for n in ("fwd_target", "fwd", "bwd")], [], [x, tgt, grad, loss]


def _backbone_configs():
    from satlas_super_resolution_amd import hip
    cfg = BACKBONE_CONFIGS
    cfg["lpips/vgg/bgr"] = (_lpips_backbone, dict(net="vgg", H=VGG_HW[0], W=VGG_HW[1]))                 # the reference's feed
    cfg["lpips/vgg/rgb+normalize"] = (_lpips_backbone, dict(net="vgg", H=VGG_HW[0], W=VGG_HW[1], bgr=False, normalize=True))
    for H, W in ((31, 31), (35, 47), (64, 64)):                   # 31: ALEXNET_MIN_SIDE, taps of 7, 3, 1, 1, 1
        cfg["lpips/alex/%dx%d" % (H, W)] = (_lpips_backbone, dict(net="alex", H=H, W=W))
    cfg["lpips/alex/31x31/refused"] = (_lpips_backbone, dict(net="alex", H=31, W=31, refused=True))
    cfg["lpips/alex/64x64/rgb+normalize"] = (_lpips_backbone, dict(net="alex", H=64, W=64, bgr=False, normalize=True))
    for mode in MODES:
        cfg["perceptual/%s" % mode] = (_perceptual_backbone, dict(mode=mode))
    for name, kw in (("conv3_4", dict(layer_weights={"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1})),
                     ("style", dict(style_weight=0.5)), ("style_only", dict(style_weight=0.5, perceptual_weight=0)),
                     ("no_input_norm", dict(use_input_norm=False)), ("range_norm", dict(range_norm=True)),
                     ("deterministic", dict(loss_flags=hip.DETERMINISTIC))):
        cfg["perceptual/fp32/%s" % name] = (_perceptual_backbone, dict(mode="fp32", **kw))


_backbone_configs()


def _sha_tensors(pairs):
    h = hashlib.sha256()
    for k, t in pairs:
        h.update(k.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def backbone_transcript(plan, launchers, weights, extra):
    """-> (text, number of C-ABI calls): every launcher, the plan's ParamStore (and a sha256 over its fp32 arena), the (key, shape, dtype)
    of every other device weight with one sha256 over the keys and bytes, the element count of every buffer the plan owns by attribute"""
    import torch
    canon = Canon([plan] + list(extra))
    out, calls = [], 0
    for name, L in launchers:
        out.append("launcher %s" % name)
        calls += fmt_launcher(canon, L, out, "  ")
    fmt_store(canon, plan.store, out)
    out.append("store data sha256 %s" % _sha_tensors([("data", plan.store.data)]))
    for k, t in weights:
        out.append("weight %s %s %s" % (k, list(t.shape), str(t.dtype).replace("torch.", "")))
    if weights:
        out.append("weights sha256 %s" % _sha_tensors(weights))
    for attr in sorted(vars(plan)):
        v = getattr(plan, attr)
        if isinstance(v, torch.Tensor) and attr != "lins":
            out.append("buffer %s numel %d" % (attr, v.numel()))
        elif isinstance(v, dict) and v and all(isinstance(t, torch.Tensor) for t in v.values()):
            out += ["buffer %s.%s numel %d" % (attr, k, v[k].numel()) for k in sorted(v)]
    return "\n".join(out) + "\n", calls


def backbone_objects(name, dev="cpu"):
    fn, kw = BACKBONE_CONFIGS[name]
    return fn(dev, **kw)


def build_backbone(name, dev="cpu"):
    """(text, calls) of one backbone configuration"""
    return backbone_transcript(*backbone_objects(name, dev))


def backbone_sweep(dev="cpu"):
    return {name: build_backbone(name, dev) for name in BACKBONE_CONFIGS}


def random_state_hashes():
    """the generator draw order of the three random states (committed fixtures and recorded figures were made with it): keys plus bytes"""
    from satlas_super_resolution_amd import lpips_metric as LM, perceptual as P
    return {"lpips_random_state(17, 'vgg')": _sha_tensors(LM.lpips_random_state(17, "vgg").items()),
            "lpips_random_state(17, 'alex')": _sha_tensors(LM.lpips_random_state(17, "alex").items()),
            "vgg19_random_state(vgg19_specs('conv5_4'), 3)": _sha_tensors(P.vgg19_random_state(P.vgg19_specs("conv5_4"), 3).items())}


def backbone_golden(runs):
    return {"configs": {k: {"calls": c, "sha256": digest(t)} for k, (t, c) in runs.items()},
            "random_states": random_state_hashes(),
            "full_text": {k: runs[k][0].splitlines() for k in BACKBONE_FULL_TEXT}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden")
    ap.add_argument("--tower-golden")
    ap.add_argument("--backbone-golden")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--setting", default="")
    ap.add_argument("--show")
    ap.add_argument("--device", default="cpu")
    a = ap.parse_args()
    if a.one:
        json.dump(sweep(a.setting, a.device), sys.stdout)
    elif a.tower_golden:
        doc = tower_golden(tower_sweep(a.device))
        with open(a.tower_golden, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print("%d tower transcripts -> %s (%d bytes)" % (len(doc["configs"]), a.tower_golden, os.path.getsize(a.tower_golden)))
    elif a.backbone_golden:
        doc = backbone_golden(backbone_sweep(a.device))
        with open(a.backbone_golden, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print("%d backbone transcripts -> %s (%d bytes)" % (len(doc["configs"]), a.backbone_golden, os.path.getsize(a.backbone_golden)))
    elif a.show in TOWER_CONFIGS:
        sys.stdout.write(build_tower(a.show, a.device)[0])
    elif a.show in BACKBONE_CONFIGS:
        sys.stdout.write(build_backbone(a.show, a.device)[0])
    elif a.show:
        name, mode = a.show.split("/")
        sys.stdout.write(build(name, mode, a.device)[0])
    else:
        doc = golden(all_runs())
        with open(a.golden, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")
        print("%d transcripts -> %s (%d bytes)" % (len(doc["configs"]), a.golden, os.path.getsize(a.golden)))
