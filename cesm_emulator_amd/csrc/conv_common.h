// What conv.hip and conv_wgrad.hip share: the geometry struct every conv kernel takes and the tap -> input pixel map.
#pragma once
#include "common.h"
#include "cesm_hip.h"

namespace {

struct ConvGeom {
  int Nb, Hi, Wi, Ho, Wo;
  int C1, C2;       // input channels from source 1 / source 2 (concat on channel axis)
  int Cout, Co1;    // output channels; [0,Co1) -> y1, [Co1,Cout) -> y2
  int KH, KW, S, P, U;
  int wch = 0;      // packed weights in the chunked layout (wpk_chunked)
};

__device__ __forceinline__ bool tap_src(const ConvGeom& g, int oy, int ox, int ky, int kx, int& iy, int& ix) {
  int ny = oy * g.S - g.P + ky;
  int nx = ox * g.S - g.P + kx;
  if (g.U != 1) {
    if ((ny % g.U) != 0 || (nx % g.U) != 0) return false;  // negative remainders are non-zero too
    ny /= g.U;
    nx /= g.U;
  }
  iy = ny;
  ix = nx;
  return (unsigned)ny < (unsigned)g.Hi && (unsigned)nx < (unsigned)g.Wi;
}

}  // namespace
