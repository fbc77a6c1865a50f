// Stand-in for the header of this name in the ATV recorder: ATVDemod includes it and uses nothing of it.
#pragma once
