// The device text of the device functors (devfn.h): what hiprtc compiles
// around the user's code. One source is
//   #define MRD_ARGS_BYTES .. [the kind's define line] kPrelude <user code> "\n" <the kind's kernels>
// and devfn.cpp's kind table says which kernels go with which functor kind.
#pragma once

namespace mrh {
namespace devfn {
namespace text {
// mrd::Bytes / Values / Emit / Text / Args / MutArgs, mrd::row and the call shims;
// expects MRD_ARGS_BYTES = sizeof(devfn::Args) to be defined in front of it
extern const char kPrelude[];
extern const char kEmitKernels[];     // map / reduce / fold (MRD_REDUCE 0 / 1 / 2)
extern const char kSortKeyKernel[];   // mr_sortkey
extern const char kCompareKernels[];  // mr_compare (MRD_CMP_T rows per tile)
extern const char kScanKernel[];      // mr_scan (MRD_SCAN_KMV 0 / 1)
extern const char kHashKernel[];      // mr_hash
extern const char kTextKernels[];     // mr_map over the records of a text
extern const char kPrintKernels[];    // mr_print (MRD_PRINT_KMV 0 / 1, MRD_TEXT_STAGE bytes of LDS stage)
}  // namespace text
}  // namespace devfn
}  // namespace mrh
