// met2_fit_nnls_lcurve.hip -- explicit instantiations of the fit kernel for one family of methods (fit_kernel.hpp); empty unless -DMET2_SPLIT_TU.
#ifdef MET2_SPLIT_TU
#define MET2_REFAC_PACKED 1    // these kernels take the packed leg of refactor_rowwise (nnls_wave.hpp)
#define MET2_ROWWALK 1        // and the row-walk changes of dual, model_signal and the wave reductions (wave_ops.hpp)
#include "fit_kernel.hpp"
template int launch_fit_nb<0, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<0, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<1, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<1, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<3, 1, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<3, 2, false>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<0, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<0, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<1, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<1, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<3, 1, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
template int launch_fit_nb<3, 2, true>(const FitArgs &, const LaunchGeom &, hipStream_t);
#endif
