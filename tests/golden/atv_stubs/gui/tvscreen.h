// Stand-in for sdrgui/gui/tvscreen.h in the ATV recorder (tests/golden/atv_rec.cpp): what TVScreen and GLShaderTVArray are to
// ATVDemod -- a bounds-checked image with a current row -- as a recording image of grey bytes.  It counts as initialised and
// starts as zeros with a null row (include/sdrx.h).  renderImage hands the event to the recorder.
#pragma once
#include <stdint.h>
#include <vector>

class TVScreen {
public:
    TVScreen() : m_cols(0), m_rows(0), m_row(-1), m_rowNeg(0), m_rowBig(0), m_colNeg(0), m_colBig(0), m_nullRow(0), m_resizes(0), m_onRender(0), m_ctx(0) {}
    void resizeTVScreen(int cols, int rows)
    {
        m_cols = cols; m_rows = rows; m_row = -1;
        m_image.assign((size_t)(cols > 0 ? cols : 0) * (size_t)(rows > 0 ? rows : 0), 0);
        m_resizes++;
    }
    bool selectRow(int line)
    {
        if (line < 0) m_rowNeg++; else if (line >= m_rows) m_rowBig++;
        if (line < m_rows && line >= 0) { m_row = line; return true; }
        m_row = -1;
        return false;
    }
    bool setDataColor(int col, int red, int green, int blue)
    {
        (void)green; (void)blue;
        if (col < 0) m_colNeg++; else if (col >= m_cols) m_colBig++;
        if (m_row < 0) m_nullRow++;
        if (col < m_cols && col >= 0 && m_row >= 0) { m_image[(size_t)m_row * m_cols + col] = (uint8_t)red; return true; }
        return false;
    }
    void renderImage(unsigned char*) { if (m_onRender) m_onRender(m_ctx); }

    int m_cols, m_rows, m_row;
    std::vector<uint8_t> m_image;
    long long m_rowNeg, m_rowBig, m_colNeg, m_colBig, m_nullRow, m_resizes;
    void (*m_onRender)(void*);
    void* m_ctx;
};
