// The MI355X as the launch rules see it.  No HIP header: the host-checked plan headers include this too.
#pragma once

namespace dasac {

constexpr int kWave = 64;          // CDNA4 wavefront
constexpr int kNumXcd = 8;         // MI355X: 8 XCDs x 32 CUs
constexpr int kNumCu = 256;

}  // namespace dasac
