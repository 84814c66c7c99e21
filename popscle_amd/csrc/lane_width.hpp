// lane_width.hpp -- the lane width of a sweep whose lanes are (entry slot, column): n columns rounded up to a power of two
// in 1..64 (64 from 33 columns on; common.hpp's DISPATCH_WIDTH names the seven values).  Plain C++ without an include:
// the plan headers that the CPU probes compile alone use it beside the units.
#pragma once
inline int lane_width(int n) {
  int W = 64;
  while (W > 1 && W / 2 >= n) W /= 2;
  return W;
}
