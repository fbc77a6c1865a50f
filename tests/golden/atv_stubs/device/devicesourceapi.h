// Stand-in for sdrbase/device/devicesourceapi.h in the ATV recorder: ATVDemod registers with it and nothing else.
#pragma once
class ThreadedBasebandSampleSink;
class ChannelSinkAPI;

class DeviceSourceAPI {
public:
    void addThreadedSink(ThreadedBasebandSampleSink*) {}
    void removeThreadedSink(ThreadedBasebandSampleSink*) {}
    void addChannelAPI(ChannelSinkAPI*) {}
    void removeChannelAPI(ChannelSinkAPI*) {}
};
