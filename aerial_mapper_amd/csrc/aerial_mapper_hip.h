// The public C ABI header (include/aerial_mapper_hip.h), reachable from this directory alone: the
// host-only headers here (amhip_dsm_plan.h, amhip_ortho_plan.h) name it, and tests/cpp/ortho_fold_emul.cc
// compiles them with nothing but this directory on its include path.
#include "../../include/aerial_mapper_hip.h"
