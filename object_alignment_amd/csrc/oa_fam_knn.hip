// oa_fam_knn.hip -- the kernels of OA_FAMILY_KNN (oa_families.hpp), explicitly instantiated, and k_bvh_knn_score; nothing else lives here.
#define OA_FAMILY_TU 1
#define OA_FAMILY_KNN_TU 1            // k_bvh_knn_score (oa_outlier.hpp) is defined in this unit
#include "oa_cluster.hpp"             // (+ oa_outlier.hpp, oa_knn.hpp, oa_bvh.hpp, oa_tri.hpp, oa_grid.hpp, oa_kernels.hpp)
#include "oa_families.hpp"
namespace oa {
OA_FAMILY_KNN()
}  // namespace oa
