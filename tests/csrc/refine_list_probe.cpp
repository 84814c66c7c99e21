// Test shim around anchor_plan::refine_modes (popscle_amd/csrc/anchor_plan.hpp), the parsing of
// `freemuxlet --anchor-refine-list FILE`.  Plain C++; nothing here touches a device (see tests/test_fmx_prior.py).
#include <cstring>

#include "anchor_plan.hpp"

extern "C" {

// ids: n sample IDs joined by '\n'.  Returns 1 and mode[n], or 0 and the unknown ID in unknown[cap]
int probe_refine_modes(int n, const char* ids, const char* listed, uint8_t* mode, char* unknown, int cap) {
  std::vector<std::string> v;
  std::istringstream in(ids);
  std::string s;
  while ((int)v.size() < n && std::getline(in, s)) v.push_back(s);
  std::vector<uint8_t> m;
  std::string bad;
  if (!anchor_plan::refine_modes(v, listed, &m, &bad)) {
    std::strncpy(unknown, bad.c_str(), (size_t)cap - 1);
    unknown[cap - 1] = 0;
    return 0;
  }
  for (size_t i = 0; i < m.size(); ++i) mode[i] = m[i];
  return 1;
}
}
