#include <hip/hip_runtime.h> /* addition.cuh includes it and uses nothing of it */
