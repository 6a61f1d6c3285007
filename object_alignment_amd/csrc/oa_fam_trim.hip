// oa_fam_trim.hip -- the kernels of OA_FAMILY_TRIM (oa_families.hpp), explicitly instantiated; nothing else lives here.
#define OA_FAMILY_TU 1
#include "oa_trim.hpp"                // (+ oa_kernels.hpp, oa_deviation.hpp's structs)
#include "oa_families.hpp"
namespace oa {
OA_FAMILY_TRIM()
}  // namespace oa
