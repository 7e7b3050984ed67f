"""The config-driven ViT tower on the device, written once for the CLIPScore metric (clipscore_metric.py, which also describes the two
families and the flat layout of a state) and the CLIP loss (clip_loss.py).  Kernels: csrc/vit.hip, vit_bwd.hip, linear_split.hip, mha_mfma.hip.

    TowerWeights   the weights, fp32, the matrices as the state_dict holds them (ssr_linear reads [Nout][K] rows), `patch.weight` as
                   [C, 3 p p] (ssr_vit_patch_input's columns) and, for `clip`, `proj.t` [E, C].  backward=True adds a transposed copy
                   `<name>.weight.t` of every matrix the backward passes through (dX = dY W is ssr_linear on W^T's rows; the probe is
                   a parameter, so pool.q has none): + 0.34 GB for ViT-B.  tower_arithmetic 'split': instead of the fp32 matrices,
                   `<key>.pk`, the packed fp16 pieces of W, and with backward=True `<name>.weight.t.pk`, the packed bf16 pieces of
                   W^T, for ssr_linear_split; a matrix with max|w| >= 64 raises ValueError by name before anything is loaded.
                   tower_attention 'mfma' changes no weight: the plans launch ssr_mha_mfma_fwd / _bwd for the blocks' self-attention;
                   the pooling head (one query row) keeps ssr_mha_fwd / _bwd.
    TowerPlan      what the static launch lists of one (B, H, W) share: the refusals, the index tables of the nearest resize (built on
                   the host with F.interpolate itself; with a backward, their inverse ranges), linear / linear_t / layernorm /
                   layernorm_bwd - where the exact | split switch lives - and forward(), one pass of the tower appended to a Launcher.

tools/plan_transcript.py (TOWER_CONFIGS) prints what both plans emit; tests/golden/tower_plans.json holds them to it."""
from __future__ import annotations

import functools
from typing import Dict

import torch

from . import hip
from .hip import F32, NULL_VIEW, View
from .linear_split import check_mfma_head_dim, check_split_domain, pack_tower

_LAYERNORMS = ("ln1", "ln2", "ln", "ln_pre", "ln_post")


class TowerWeights:
    """`where` begins every refusal: "train.clip_opt" | "metric type 'calculate_clipscore'".  The option values arrive checked."""

    def __init__(self, state: Dict[str, torch.Tensor], device, gelu: str, tower_arithmetic: str, tower_attention: str, where: str,
                 backward: bool = False):
        from .clipscore_metric import _flat_keys, vit_config_from_state
        self.cfg = vit_config_from_state(state)
        self.device, self.gelu, self.where, self.backward = torch.device(device), gelu, where, backward
        self.tower_arithmetic, self.tower_attention = tower_arithmetic, tower_attention
        clip, split = self.cfg["family"] == "clip", tower_arithmetic == "split"
        keys = _flat_keys(self.cfg["family"], self.cfg["depth"])
        for k in keys:
            if k not in state:
                raise KeyError(k)
        mats = [k for k in keys if k.endswith(".weight") and k.split(".")[-2] not in _LAYERNORMS]
        if split:
            check_split_domain([(k, state[k]) for k in mats] + ([("proj", state["proj"])] if clip else []), where)
        w = self.w = {k: v.detach().to(torch.float32).contiguous().to(self.device) for k, v in state.items() if k not in ("heads", "image_size")}
        w["patch.weight"] = w["patch.weight"].reshape(self.cfg["width"], -1)
        if clip:
            w["proj.t"] = w["proj"].t().contiguous()
            mats.append("proj.t")
        transposed = [k for k in mats if k != "pool.q.weight"] if backward else []
        if split:
            pack_tower(w, mats, transposed)
            for k in mats:
                del w[k]
        else:
            for k in transposed:
                w[f"{k}.t"] = w[k].t().contiguous()
        self.act = hip.VIT_ACTS["quick_gelu" if clip else f"gelu_{gelu}"]


class TowerPlan:
    """`subject` names the plan in the refusal of an empty batch: "CLIPScore" | "the CLIP loss"."""

    def __init__(self, model: TowerWeights, B: int, H: int, W: int, subject: str):
        from .clipscore_metric import nearest_index_table
        cfg = model.cfg
        if B <= 0 or H <= 0 or W <= 0:
            raise ValueError(f"{subject} needs at least one image, got {B} x {H} x {W}")
        p, g, d, S = (cfg[k] for k in ("patch", "grid", "head_dim", "image_size"))
        if p % 2:
            raise ValueError(f"patch size {p}: ssr_linear contracts 3 p^2 channels, a multiple of 4")
        if model.backward and d not in (64, 72):
            raise NotImplementedError(f"{model.where}: head dim {d} has no attention backward (ssr_mha_bwd: 64, 72)")
        if model.tower_attention == "mfma":
            check_mfma_head_dim(d, model.where)
        self.model, self.B, self.H, self.W, self.lib, self.Cw, self.eps = model, B, H, W, hip.lib(), cfg["width"], cfg["ln_eps"]
        i32 = lambda t: t.to(torch.int32).contiguous().to(model.device)      # noqa: E731
        # the resize to S x S, of which the patch convolution reads the first g * p rows and columns
        self.rowidx, self.colidx = i32(nearest_index_table(H, S)[:g * p]), i32(nearest_index_table(W, S)[:g * p])
        if model.backward:
            from .clip_loss import nearest_inverse_ranges
            self.rowrange, self.colrange = i32(nearest_inverse_ranges(H, S, g * p)), i32(nearest_inverse_ranges(W, S, g * p))

    def ptr(self, key: str) -> int:
        return self.model.w[key].data_ptr()

    def _product(self, L, xv, wkey, bias, res, yv, pieces, rows, K, Nout, act, what):
        if self.model.tower_arithmetic == "split":
            L.add(self.lib.ssr_linear_split, xv, self.ptr(f"{wkey}.pk"), bias, res, yv, pieces, rows, K, Nout, act, what=what)
        else:
            L.add(self.lib.ssr_linear, xv, self.ptr(wkey), bias, res, yv, F32, rows, K, Nout, act, what=what)

    def linear(self, L, xv, name, yv, rows, K, Nout, act=0, res=NULL_VIEW, wkey=None, bias=True):
        """Y [rows, Nout] = act(X [rows, K] W^T + bias) + res; split: fp16 pieces"""
        self._product(L, xv, wkey or f"{name}.weight", self.ptr(f"{name}.bias") if bias else None, res, yv, hip.SPLIT_F16, rows, K, Nout,
                      act, f"linear {name}")

    def linear_t(self, L, dyv, name, dxv, rows, K, Nout):
        """dX [rows, Nout] = dY [rows, K] W, W = `name`.weight [K, Nout]; split: bf16 pieces"""
        self._product(L, dyv, f"{name}.weight.t", None, NULL_VIEW, dxv, hip.SPLIT_BF16, rows, K, Nout, 0, f"linear^T {name}")

    def layernorm(self, L, xv, name, yv, rows):
        L.add(self.lib.ssr_layernorm_fwd, xv, self.ptr(f"{name}.weight"), self.ptr(f"{name}.bias"), yv, F32, rows, self.Cw, self.eps,
              what=f"layernorm {name}")

    def layernorm_bwd(self, L, xv, name, dyv, rv, outv, rows):
        L.add(self.lib.ssr_layernorm_bwd, xv, self.ptr(f"{name}.weight"), dyv, rv, outv, F32, rows, self.Cw, self.eps, what=f"layernorm bwd {name}")

    def split(self, t: torch.Tensor, n: int):
        """the n width-C slices of a packed [rows, n C] buffer"""
        return [View(t.data_ptr(), n * self.Cw, i * self.Cw) for i in range(n)]

    def forward(self, L, add_input, s, xs, qkvs, xmids, pres, head, feat):
        """One pass appended to L: the caller's input stage, the patch embedding, ssr_vit_tokens, per block ln1 / qkv / attention over
        the slices of the packed buffer / proj (+ residual) / ln2 / fc1, activation / fc2 (+ residual), then the family's pooling.
          add_input(L, patches)  adds the launch that fills the view `patches` [B G, 3 p p]
          s        scratch shared by a plan's passes: patches, embed [B G, C], h, att [M, C], post [M, mlp]; siglip: probe, pa, pz [B, C],
                   pm [B, mlp]; clip: pooled [B, C]
          xs       depth + 1 row buffers [M, C]: every block's input, then the last rows (one buffer throughout: rows updated in place)
          qkvs, xmids  per block: the packed qkv [M, 3 C] and the rows after the attention's residual
          pres     per block, where fc1 keeps its pre-activation for ssr_vit_act_fwd to take into s["post"]; None: the activation is
                   fused into fc1, which writes s["post"]
          head     siglip: (q [B, C], kv [M, 2 C], py [B, C], ppre [B, mlp] or None, as `pres`), the pooling head's own buffers
          feat     [B, out_dim]"""
        model, lib, B, Cw = self.model, self.lib, self.B, self.Cw
        fam, p, g, T, mlp, heads, d, E, depth = (model.cfg[k] for k in ("family", "patch", "grid", "tokens", "mlp", "heads", "head_dim", "out_dim", "depth"))
        G, M, KP, scale = g * g, B * T, 3 * p * p, float(d) ** -0.5
        mha_blocks = lib.ssr_mha_mfma_fwd if model.tower_attention == "mfma" else lib.ssr_mha_fwd      # the pooling head keeps ssr_mha_fwd
        view, split = functools.lru_cache(None)(hip.view), functools.lru_cache(None)(self.split)        # one record per buffer, not per launch

        def mlp_of(xv, name, pre, post, yv, rows, res):
            if pre is None:
                self.linear(L, xv, f"{name}.fc1", view(post), rows, Cw, mlp, act=model.act)
            else:                                      # same device function as the fused form: same bytes
                self.linear(L, xv, f"{name}.fc1", view(pre), rows, Cw, mlp)
                L.add(lib.ssr_vit_act_fwd, view(pre), view(post), F32, rows, mlp, model.act, what=f"activation {name}")
            self.linear(L, view(post), f"{name}.fc2", yv, rows, mlp, Cw, res=res)

        add_input(L, view(s["patches"]))
        self.linear(L, view(s["patches"]), "patch", view(s["embed"]), B * G, KP, Cw, bias=fam == "siglip")
        L.add(lib.ssr_vit_tokens, view(s["embed"]), self.ptr("cls") if fam == "clip" else None, self.ptr("pos"), view(xs[0]), F32, B, G, Cw, what="tokens")
        hv = view(s["h"])
        if fam == "clip":
            self.layernorm(L, view(xs[0]), "ln_pre", view(xs[0]), M)
        for i in range(depth):
            n = f"blocks.{i}"
            qs = split(qkvs[i], 3)
            self.layernorm(L, view(xs[i]), f"{n}.ln1", hv, M)
            self.linear(L, hv, f"{n}.qkv", view(qkvs[i]), M, Cw, 3 * Cw)
            L.add(mha_blocks, qs[0], qs[1], qs[2], view(s["att"]), F32, B, T, T, heads, d, scale, what=f"attention {n}")
            self.linear(L, view(s["att"]), f"{n}.proj", view(xmids[i]), M, Cw, Cw, res=view(xs[i]))
            self.layernorm(L, view(xmids[i]), f"{n}.ln2", hv, M)
            mlp_of(hv, n, pres and pres[i], s["post"], view(xs[i + 1]), M, view(xmids[i]))
        if fam == "clip":
            self.layernorm(L, View(xs[depth].data_ptr(), T * Cw, 0), "ln_post", view(s["pooled"]), B)      # the class-token row of every image
            self.linear(L, view(s["pooled"]), "proj", view(feat), B, Cw, E, wkey="proj.t", bias=False)
            return
        q, kv, py, ppre = head
        ks = split(kv, 2)
        self.layernorm(L, view(xs[depth]), "ln_post", hv, M)
        self.linear(L, view(s["probe"]), "pool.q", view(q), B, Cw, Cw)
        self.linear(L, hv, "pool.kv", view(kv), M, Cw, 2 * Cw)
        L.add(lib.ssr_mha_fwd, view(q), ks[0], ks[1], view(s["pa"]), F32, B, 1, T, heads, d, scale, what="attention pool")
        self.linear(L, view(s["pa"]), "pool.proj", view(py), B, Cw, Cw)
        self.layernorm(L, view(py), "pool.ln", view(s["pz"]), B)
        mlp_of(view(s["pz"]), "pool", ppre, s["pm"], view(feat), B, view(py))
