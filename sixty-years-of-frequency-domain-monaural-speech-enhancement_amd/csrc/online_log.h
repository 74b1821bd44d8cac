// Launch record of launch_tcm_chain (k_tcm_stream.hip), for tests that must know which instance of the chain kernel a launch
// reached (csrc/tests/online_probe.hip).  Kept apart from the norm launch log (kernels.h), whose readers list the norm passes of a
// call exactly.  Host-side only: nothing the kernel computes depends on it.
#pragma once
#include "kernels.h"

namespace se {

// nullptr (the default): nothing is recorded.  Otherwise every launch_tcm_chain on this thread appends its record (NormLaunchRec:
// kernel "tcm_chain", grid, block, shmem; KS = taps of the chain's dilated conv, the kernel's template argument).
void online_set_launch_log(std::vector<NormLaunchRec>* log);

}  // namespace se
