// frames_view.hip -- the view kernels of frames.hip (Viewed<Source> of the six sources, their check and launchers) as a translation unit
// of their own: the kernels of frames.hip are then compiled exactly as without them.
#define FRAMES_VIEW_TU 1
#include "frames.hip"
