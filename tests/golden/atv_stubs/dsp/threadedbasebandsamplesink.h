// Stand-in for sdrbase/dsp/threadedbasebandsamplesink.h in the ATV recorder: the recorder calls feed() itself.
#pragma once
#include <QObject>
class BasebandSampleSink;

class ThreadedBasebandSampleSink {
public:
    ThreadedBasebandSampleSink(BasebandSampleSink*, QObject* = 0) {}
};
