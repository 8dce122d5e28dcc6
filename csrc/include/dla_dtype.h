// Element type codes of the launchers: what the bindings pass down and the kernel files dispatch on.
#pragma once

namespace dla {

enum DType : int { kF32 = 0, kBF16 = 1 };

}  // namespace dla
