// Private to csrc: the weights blob -> the operand tables of a handle (weight_pack.hip).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "bp_context.h"

namespace bp {

// What bp_create takes from the weights blob: the scalars, and per device table the handle field it fills and its bytes.
struct PackedWeights {
  LogConsts kc{};
  float b_contour2 = 0, b_note2 = 0, b_onset2 = 0;
  std::vector<std::pair<bp_context::Table bp_context::*, std::vector<uint8_t>>> tables;
};

// Parses and checks the blob and packs every operand table `flags` (BP_FLAG_*) needs.  Host only: touches no device.
// Returns BP_OK, or bp_create's error code with the message in `err`.
int pack_weights(const void* blob, size_t nbytes, unsigned flags, PackedWeights& out, std::string& err);

}  // namespace bp
