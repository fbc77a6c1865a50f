// Stand-in for sdrbase/dsp/downchannelizer.h in the ATV recorder: the notification ATVDemod::handleMessage takes the channel
// rate and the offset from, and the calls it makes on the channelizer.  A BasebandSampleSink, as the real one is.
#pragma once
#include "dsp/basebandsamplesink.h"
#include "util/message.h"
#include "util/messagequeue.h"

class DownChannelizer : public BasebandSampleSink {
public:
    class MsgChannelizerNotification : public Message {
        MESSAGE_CLASS_DECLARATION
    public:
        MsgChannelizerNotification(int sampleRate, qint64 frequencyOffset) : Message(), m_sampleRate(sampleRate), m_frequencyOffset(frequencyOffset) {}
        int getSampleRate() const { return m_sampleRate; }
        qint64 getFrequencyOffset() const { return m_frequencyOffset; }
    private:
        int m_sampleRate;
        qint64 m_frequencyOffset;
    };
    DownChannelizer(BasebandSampleSink*) {}
    virtual void start() {}
    virtual void stop() {}
    virtual void feed(const SampleVector::const_iterator&, const SampleVector::const_iterator&, bool) {}
    virtual bool handleMessage(const Message&) { return false; }
    void configure(MessageQueue*, int, int) {}
    int getInputSampleRate() const { return 0; }
};
