// gaussian_hmm.h -- the dimension limits of the Kalman filter / smoother kernel (gaussian_hmm.hip).  Larger
// dimensions return PA_ERR_UNSUPPORTED; the Python class then takes its torch route.
#pragma once

namespace pa {

constexpr int GH_MAXHIDDEN = 16;
constexpr int GH_MAXOBS = 16;

}  // namespace pa
