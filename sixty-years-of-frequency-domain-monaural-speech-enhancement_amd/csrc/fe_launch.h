// Form of one dispatch of the two transforms, for tests that must know which template instance a launch asks for
// (csrc/tests/fe_probe.hip).  Host-side only: nothing the kernels compute depends on it.
#pragma once
#include <vector>

namespace se {

struct FeLaunchRec {
    const char* kernel = "";     // "stft2" (stft2_kernel<N, MAG, CP>) or "istft2" (istft2_kernel<N, FSC>)
    int N = 0, MAG = 0, CP = 0, FSC = 0;
    int gx = 0, gy = 0, block = 0;
    long shmem = 0;              // dynamic LDS bytes
    int ragged = 0;              // the launch reads the published per-row sizes
};
// nullptr (the default): nothing is recorded.  Otherwise launch_stft and launch_istft on this thread append their record.
void fe_set_launch_log(std::vector<FeLaunchRec>* log);
std::vector<FeLaunchRec>* fe_launch_log();

}  // namespace se
