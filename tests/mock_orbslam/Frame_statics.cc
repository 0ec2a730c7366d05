// TEST INFRASTRUCTURE ONLY -- the static data members of the mock ORB_SLAM2::Frame, defined once; linked into every shim program.
#include "Frame.h"
namespace ORB_SLAM2 {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
bool Frame::mbUArucoIni = false;
}
