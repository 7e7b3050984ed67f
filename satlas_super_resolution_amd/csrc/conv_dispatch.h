// Host-side dispatch of ssr_conv2d: one record per kernel family, defined by the family's file.  conv.hip keeps one ordered candidate
// list per dtype and one select() behind ssr_conv2d, ssr_conv2d_impl, ssr_conv2d_variant and ssr_conv2d_symbol.
#pragma once
#include "common.h"
#include <cstdio>

// (plain variables with const members, not `const` objects: hipcc emits a constant-initialised const object into the device code
// object as well, where the host functions it points to do not exist)
struct ssr_conv_family {
    const char* const name;  // "thin", "ws", "big", "bigx3", "x3r", "x3q", "res", "pipelined"
    const int impl;          // the ssr_conv2d_impl code that forces the family; -1: cannot be forced (tried by every code but 3)
    bool (*const shape_ok)(const ssr_conv_desc&);            // what the kernel can run at all (a forced launch needs only this)
    bool (*const qualifies)(const ssr_conv_desc&);           // shape_ok + off switch + grid heuristic: chosen by itself
    int (*const launch)(const ssr_conv_desc&, hipStream_t);  // of a descriptor that passed shape_ok
    int (*const code)(const ssr_conv_desc&);                 // the two low digits of ssr_conv2d_variant: NT * 10 + the family's digit
    // the kernel symbol `launch` starts, as rocprofv3 prints it; v = the whole variant code (ssr_conv_symbol_coded prints it)
    void (*const symbol)(const ssr_conv_desc&, int v, char* buf, int buflen);
};
// thin-output VALU (conv_thin.hip), weight-stationary (conv_ws.hip), big tile (conv_big.hip; split modes: conv_big_x3.hip), register-tiled
// (conv_x3r.hip), twelve-wave ring (conv_x3q.hip), K-resident (conv_res.hip); the pipelined family is conv.hip's own
extern ssr_conv_family ssr_conv_thin, ssr_conv_ws, ssr_conv_big, ssr_conv_bigx3, ssr_conv_x3r, ssr_conv_x3q, ssr_conv_res;

// n <= 4 parity-class descriptors (2x2 stride 1, identical geometry) in ONE big-tile launch; false: not taken, nothing launched
bool ssr_conv_big_batch_try(const ssr_conv_desc* ds, int n, hipStream_t st, int* rc);
bool ssr_conv_bigx3_batch_try(const ssr_conv_desc* ds, int n, hipStream_t st, int* rc);

// the instantiation conv_x3r_kernel<NTW, NU, EP, TH, AM> the register-tiled family launches (the chain kernel, conv_x3c.hip, shares EP)
struct ssr_conv_x3r_instance { int ntw, nu, ep, th, am; };
ssr_conv_x3r_instance ssr_conv_x3r_pick(const ssr_conv_desc& d);

template <int CODE> int ssr_conv_code(const ssr_conv_desc&) { return CODE; }
// "kernel<dtype,K,S,NT,W>": the families whose template lists follow internal tile choices are filed under their name and variant code
inline void ssr_conv_symbol_coded(const char* kernel, const ssr_conv_desc& d, int v, char* buf, int buflen) {
    const char* dt = d.dtype == SSR_BF16 ? "bf16" : d.dtype == SSR_F32 ? "fp32" : d.dtype == SSR_F32H ? "fp32h" : "fp32x3";
    snprintf(buf, buflen, "%s<%s,K%d,S%d,NT%d,W%d>", kernel, dt, v / 1000, (v / 100) % 10, (v / 10) % 10, v % 10);
}
